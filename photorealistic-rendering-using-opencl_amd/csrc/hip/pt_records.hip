// pt_records.hip -- denoiser inputs as records (prt_export_denoise_inputs, prt_denoise_records; include/prt.h has the contract).
// A translation unit of its own: no code object of the render kernels, of pt_denoise.hip or of pt_temporal.hip changes with it.
//
//   rec_export_kernel   per pixel of a frame part: framebuffer word, the two guide words and {v of the stats plane, has_stats, 0, 0} into
//                       one 64-byte record
//   rec_import_kernel   per pixel of a gathered frame: the record back into the planes the filter reads (framebuffer, guides, {rgb, v}) and
//                       "a record without stats" into a flag word
//
// 16x16 workgroups, one lane per pixel like the filter's kernels; a lane moves its record as four float4 (64 contiguous bytes, a wave's
// rows are contiguous runs of 1 KiB).  Both kernels are copies with a handful of flops: 112 bytes per pixel, memory bound.
#include "pt_denoise_dev.h"
#include "pt_launch.h"

namespace prt {

// adapt null: the frame has no stats plane that belongs to its picture (v = 0, has_stats = 0).  v is dn_var_kernel's (pt_denoise.hip):
// dn_stats_var
__global__ __launch_bounds__(256) void rec_export_kernel(const float4* __restrict__ fb, const uint4* __restrict__ q4,
                                                         const float2* __restrict__ adapt, const float4* __restrict__ gd, int W, int H,
                                                         float4* __restrict__ rec) {
    const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t id = (size_t)y * W + x;
    const float v = adapt ? dn_stats_var(q4, adapt, id) : 0.0f;
    rec[4 * id] = fb[id];
    rec[4 * id + 1] = gd[2 * id];
    rec[4 * id + 2] = gd[2 * id + 1];
    rec[4 * id + 3] = make_float4(v, adapt ? 1.0f : 0.0f, 0.0f, 0.0f);
}

// no_stats: every lane that finds a record without stats stores the same 1 (a plain store: no atomics, no order needed)
__global__ __launch_bounds__(256) void rec_import_kernel(const float4* __restrict__ rec, int W, int H, float4* __restrict__ fb,
                                                         float4* __restrict__ gd, float4* __restrict__ var, unsigned* __restrict__ no_stats) {
    const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t id = (size_t)y * W + x;
    const float4 c = rec[4 * id], s = rec[4 * id + 3];
    fb[id] = c;
    gd[2 * id] = rec[4 * id + 1];
    gd[2 * id + 1] = rec[4 * id + 2];
    var[id] = make_float4(c.x, c.y, c.z, s.x);
    if (!(s.y == 1.0f)) *no_stats = 1u;
}

void launch_records_export(const float4* fb, const uint4* q4, const float2* adapt, const float4* guides, int W, int rows, float4* records,
                           hipStream_t stream) {
    hipLaunchKernelGGL(rec_export_kernel, dn_grid(W, rows), dn_block(), 0, stream, fb, q4, adapt, guides, W, rows, records);
}
void launch_records_import(const float4* records, int W, int H, float4* fb, float4* guides, float4* var, unsigned* no_stats, hipStream_t stream) {
    hipLaunchKernelGGL(rec_import_kernel, dn_grid(W, H), dn_block(), 0, stream, records, W, H, fb, guides, var, no_stats);
}

}  // namespace prt
