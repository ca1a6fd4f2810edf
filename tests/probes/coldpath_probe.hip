// tests/probes/coldpath_probe.hip -- TEST INFRASTRUCTURE, never part of libprt.
//
// One kernel per exact fast path of csrc/hip/pt_device.h: load a value, apply the helper, store the result.  tests/test_codegen_coldpaths.py
// compiles this to a listing (no GPU) and checks the shape of each: one scalar branch to the IEEE block, nothing exec-masked.
#include <hip/hip_runtime.h>

#include "pt_device.h"

using namespace prt::dev;

extern "C" __global__ void probe_recip(const float* __restrict__ in, float* __restrict__ out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = hw_recip(in[i]);
}
extern "C" __global__ void probe_sqrt(const float* __restrict__ in, float* __restrict__ out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = hw_sqrt(in[i]);
}
extern "C" __global__ void probe_unit_range(const float* __restrict__ in, float* __restrict__ out, float c, float u) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = out_of_unit_range(in[i], c, u) ? 1.0f : 0.0f;
}
extern "C" __global__ void probe_sincos(const float* __restrict__ in, float* __restrict__ out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    float s, c;
    sincos_pair(in[i], s, c);
    out[2u * i] = s;
    out[2u * i + 1u] = c;
}
