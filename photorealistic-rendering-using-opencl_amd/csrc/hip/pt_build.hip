// pt_build.hip -- prt_rebuild_bvh on the device (prt.h): new vertices -> a Morton-order tree over all T triangles, written as the tables a refit
// reads; pt_refit.hip then makes the records and the boxes.  Wave64 streaming kernels of 256 lanes around the bodies of pt_build.h.  The
// project's own kernels wait on no other workgroup: every stage reads only what launches that have ended wrote (the extent is reduced in two
// launches, no float atomics; the only atomic is an integer max).  The two sorts and the scan are rocPRIM's, which may use decoupled look-back
// inside (DESIGN.md s4 "Rebuild").
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "pt_build.h"
#include "pt_launch.h"

namespace prt {

// the six lo / hi values of 256 lanes -> lane 0's
__device__ inline void build_block_reduce(float lo[3], float hi[3], float (*s)[256]) {
    const unsigned t = threadIdx.x;
    for (int k = 0; k < 3; ++k) { s[k][t] = lo[k]; s[3 + k][t] = hi[k]; }
    __syncthreads();
    for (unsigned w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            float lo2[3], hi2[3];
            for (int k = 0; k < 3; ++k) { lo[k] = s[k][t]; hi[k] = s[3 + k][t]; lo2[k] = s[k][t + w]; hi2[k] = s[3 + k][t + w]; }
            build_extent_merge(lo, hi, lo2, hi2);
            for (int k = 0; k < 3; ++k) { s[k][t] = lo[k]; s[3 + k][t] = hi[k]; }
        }
        __syncthreads();
    }
}

// stage 1a: one lane per triangle, one partial {lo[3], hi[3]} of the centres per block (a lane past the end repeats the last triangle)
__global__ __launch_bounds__(256) void build_extent_kernel(const float* __restrict__ vertices, uint32_t n_tris, float* __restrict__ partials) {
    __shared__ float s[6][256];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    float c[3], lo[3], hi[3];
    build_centre(vertices, i < n_tris ? i : n_tris - 1u, c);
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = c[k];
    build_block_reduce(lo, hi, s);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) { partials[6 * (size_t)blockIdx.x + k] = lo[k]; partials[6 * (size_t)blockIdx.x + 3 + k] = hi[k]; }
}

// stage 1b: one block over the partials
__global__ __launch_bounds__(256) void build_extent_final_kernel(const float* __restrict__ partials, uint32_t n_partials, BuildExtent* __restrict__ extent) {
    __shared__ float s[6][256];
    float lo[3], hi[3];
    const uint32_t p0 = threadIdx.x < n_partials ? threadIdx.x : n_partials - 1u;
    for (int k = 0; k < 3; ++k) { lo[k] = partials[6 * (size_t)p0 + k]; hi[k] = partials[6 * (size_t)p0 + 3 + k]; }
    for (uint32_t p = threadIdx.x + 256u; p < n_partials; p += 256u) build_extent_merge(lo, hi, partials + 6 * (size_t)p, partials + 6 * (size_t)p + 3);
    build_block_reduce(lo, hi, s);
    if (threadIdx.x == 0) *extent = build_extent_finish(lo, hi);
}

// stage 2: one lane per triangle
__global__ __launch_bounds__(256) void build_key_kernel(const float* __restrict__ vertices, uint32_t n_tris, const BuildExtent* __restrict__ extent,
                                                        uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tris) return;
    const BuildExtent e = *extent;
    keys[i] = build_key(vertices, i, e);
}

// stage 3: one lane per inner node of the radix tree
__global__ __launch_bounds__(256) void build_node_kernel(const uint64_t* __restrict__ keys, uint32_t n_keys, BuildNode* __restrict__ nodes,
                                                         uint32_t* __restrict__ parent) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i + 1u >= n_keys) return;
    build_node(keys, n_keys, i, nodes, parent);
}

// stage 4: one lane per inner node: its sort key, its own index as the value, and the largest count of pairs with two inner children
__global__ __launch_bounds__(256) void build_pair_key_kernel(const BuildNode* __restrict__ nodes, const uint32_t* __restrict__ parent, uint32_t n,
                                                             uint32_t max_leaf, uint64_t* __restrict__ pair_keys, uint32_t* __restrict__ order,
                                                             BuildHeader* hdr) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        uint32_t two;
        pair_keys[i] = build_pair_key(nodes, parent, i, max_leaf, &two);
        order[i] = i;
        if (two) atomicMax(&s_max, two);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(&hdr->max_two, s_max);
}

// stage 5a: one lane per position of the sorted pair keys
__global__ __launch_bounds__(256) void build_number_kernel(const uint64_t* __restrict__ pair_keys, const uint32_t* __restrict__ order, uint32_t n,
                                                           const BuildNode* __restrict__ nodes, uint32_t max_leaf, uint32_t* __restrict__ pair_of,
                                                           uint32_t* __restrict__ leaf_tris, BuildHeader* hdr) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    build_number(pair_keys, order, n, k, nodes, max_leaf, pair_of, leaf_tris, hdr);
}

// stage 5b: one lane per position again, behind the scan of leaf_tris
__global__ __launch_bounds__(256) void build_pair_kernel(const uint64_t* __restrict__ pair_keys, const uint32_t* __restrict__ order, uint32_t n,
                                                         const BuildNode* __restrict__ nodes, const uint32_t* __restrict__ pair_of,
                                                         const uint32_t* __restrict__ slot_base, const uint64_t* __restrict__ tri_keys,
                                                         uint32_t max_leaf, NodePair* __restrict__ pairs, uint32_t* __restrict__ slot_vtx,
                                                         uint32_t* __restrict__ level_pairs) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    build_pair(pair_keys, order, k, nodes, pair_of, slot_base, tri_keys, max_leaf, pairs, slot_vtx, level_pairs);
}

__global__ __launch_bounds__(256) void build_root_slot_kernel(const uint64_t* __restrict__ tri_keys, uint32_t n_tris, uint32_t* __restrict__ slot_vtx) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_tris) build_root_slot(tri_keys, s, slot_vtx);
}

__global__ __launch_bounds__(256) void build_old_slot_kernel(const uint32_t* __restrict__ old_slot_vtx, uint32_t n_old_slots, uint32_t n_tris,
                                                             uint32_t* __restrict__ old_slot) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_old_slots && old_slot_vtx[s] / 3u < n_tris) build_old_slot(old_slot_vtx, s, old_slot);
}

// a triangle without an old slot sets the flag word (every lane that stores writes the same value)
__global__ __launch_bounds__(256) void build_missing_kernel(const uint32_t* __restrict__ old_slot, uint32_t n_tris, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_tris && old_slot[i] == PT_BUILD_NONE) *flag = 1u;
}

__global__ __launch_bounds__(256) void build_carry_kernel(const uint32_t* __restrict__ slot_vtx, uint32_t n_slots, const uint32_t* __restrict__ old_slot,
                                                          int carry_nrm, const TriNrm* __restrict__ nrm_old, TriNrm* __restrict__ nrm_new,
                                                          const TriGeom* __restrict__ prev_old, const TriGeom* __restrict__ geom_new,
                                                          TriGeom* __restrict__ prev_new) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_slots) build_carry(slot_vtx, s, old_slot, carry_nrm != 0, nrm_old, nrm_new, prev_old, geom_new, prev_new);
}

static inline dim3 blocks_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

hipError_t build_work_layout(uint32_t T, void* base, BuildWork& w, size_t* bytes) {
    const size_t n = T > 1u ? T - 1u : 1u, parts = ((size_t)T + 255) / 256;
    size_t t_keys = 0, t_pairs = 0, t_scan = 0;
    hipError_t e;
    uint64_t* k64 = nullptr;
    uint32_t* k32 = nullptr;
    if ((e = rocprim::radix_sort_keys(nullptr, t_keys, k64, k64, (size_t)T, 0u, 62u, (hipStream_t)0)) != hipSuccess) return e;
    if ((e = rocprim::radix_sort_pairs(nullptr, t_pairs, k64, k64, k32, k32, n, 0u, 39u, (hipStream_t)0)) != hipSuccess) return e;
    if ((e = rocprim::exclusive_scan(nullptr, t_scan, k32, k32, 0u, n, rocprim::plus<uint32_t>(), (hipStream_t)0)) != hipSuccess) return e;
    w.temp_bytes = t_keys > t_pairs ? t_keys : t_pairs;
    if (t_scan > w.temp_bytes) w.temp_bytes = t_scan;
    if (!w.temp_bytes) w.temp_bytes = 256;
    char* p = static_cast<char*>(base);
    size_t at = 0;
    auto take = [&](size_t b) { char* r = p ? p + at : nullptr; at += up256(b); return r; };
    w.keys = reinterpret_cast<uint64_t*>(take(8 * (size_t)T));
    w.keys_sorted = reinterpret_cast<uint64_t*>(take(8 * (size_t)T));
    w.pair_keys = reinterpret_cast<uint64_t*>(take(8 * n));
    w.pair_keys_sorted = reinterpret_cast<uint64_t*>(take(8 * n));
    w.nodes = reinterpret_cast<BuildNode*>(take(sizeof(BuildNode) * n));
    w.parent = reinterpret_cast<uint32_t*>(take(4 * n));
    w.order_in = reinterpret_cast<uint32_t*>(take(4 * n));
    w.order = reinterpret_cast<uint32_t*>(take(4 * n));
    w.pair_of = reinterpret_cast<uint32_t*>(take(4 * n));
    w.leaf_tris = reinterpret_cast<uint32_t*>(take(4 * n));
    w.slot_base = reinterpret_cast<uint32_t*>(take(4 * n));
    w.old_slot = reinterpret_cast<uint32_t*>(take(4 * (size_t)T));
    w.partials = reinterpret_cast<float*>(take(24 * parts));
    w.extent = reinterpret_cast<BuildExtent*>(take(sizeof(BuildExtent)));
    w.hdr = reinterpret_cast<BuildHeader*>(take(sizeof(BuildHeader)));
    w.flags = reinterpret_cast<uint32_t*>(take(16));
    w.temp = take(w.temp_bytes);
    *bytes = at;
    return hipSuccess;
}

void launch_build_old_slots(const BuildWork& w, const uint32_t* old_slot_vtx, size_t n_old_slots, uint32_t T, bool check_missing, hipStream_t stream) {
    (void)hipMemsetAsync(w.old_slot, 0xFF, 4 * (size_t)T, stream);
    if (n_old_slots)
        hipLaunchKernelGGL(build_old_slot_kernel, blocks_of(n_old_slots), dim3(256), 0, stream, old_slot_vtx, (uint32_t)n_old_slots, T, w.old_slot);
    if (check_missing) hipLaunchKernelGGL(build_missing_kernel, blocks_of(T), dim3(256), 0, stream, w.old_slot, T, w.flags + 1);
}

hipError_t launch_build_tree(const BuildWork& w, const float* vertices, uint32_t T, uint32_t max_leaf, NodePair* pairs, uint32_t* slot_vtx,
                             uint32_t* level_pairs, hipStream_t stream) {
    hipError_t e;
    const uint32_t parts = (T + 255u) / 256u;
    hipLaunchKernelGGL(build_extent_kernel, dim3(parts), dim3(256), 0, stream, vertices, T, w.partials);
    hipLaunchKernelGGL(build_extent_final_kernel, dim3(1), dim3(256), 0, stream, w.partials, parts, w.extent);
    hipLaunchKernelGGL(build_key_kernel, dim3(parts), dim3(256), 0, stream, vertices, T, w.extent, w.keys);
    size_t tb = w.temp_bytes;
    if ((e = rocprim::radix_sort_keys(w.temp, tb, w.keys, w.keys_sorted, (size_t)T, 0u, 62u, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.hdr, 0, sizeof(BuildHeader), stream)) != hipSuccess) return e;
    if (T <= max_leaf) {
        hipLaunchKernelGGL(build_root_slot_kernel, dim3(parts), dim3(256), 0, stream, w.keys_sorted, T, slot_vtx);
        return hipGetLastError();
    }
    const uint32_t n = T - 1u;
    hipLaunchKernelGGL(build_node_kernel, blocks_of(n), dim3(256), 0, stream, w.keys_sorted, T, w.nodes, w.parent);
    hipLaunchKernelGGL(build_pair_key_kernel, blocks_of(n), dim3(256), 0, stream, w.nodes, w.parent, n, max_leaf, w.pair_keys, w.order_in, w.hdr);
    tb = w.temp_bytes;
    if ((e = rocprim::radix_sort_pairs(w.temp, tb, w.pair_keys, w.pair_keys_sorted, w.order_in, w.order, (size_t)n, 0u, 39u, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(build_number_kernel, blocks_of(n), dim3(256), 0, stream, w.pair_keys_sorted, w.order, n, w.nodes, max_leaf, w.pair_of, w.leaf_tris, w.hdr);
    tb = w.temp_bytes;
    if ((e = rocprim::exclusive_scan(w.temp, tb, w.leaf_tris, w.slot_base, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(build_pair_kernel, blocks_of(n), dim3(256), 0, stream, w.pair_keys_sorted, w.order, n, w.nodes, w.pair_of, w.slot_base, w.keys_sorted,
                       max_leaf, pairs, slot_vtx, level_pairs);
    return hipGetLastError();
}

void launch_build_carry(const BuildWork& w, const uint32_t* slot_vtx, uint32_t n_slots, bool carry_nrm, const TriNrm* nrm_old, TriNrm* nrm_new,
                        const TriGeom* prev_old, const TriGeom* geom_new, TriGeom* prev_new, hipStream_t stream) {
    hipLaunchKernelGGL(build_carry_kernel, blocks_of(n_slots), dim3(256), 0, stream, slot_vtx, n_slots, w.old_slot, carry_nrm ? 1 : 0, nrm_old, nrm_new,
                       prev_old, geom_new, prev_new);
}

}  // namespace prt
