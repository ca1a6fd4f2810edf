// tests/probes/sincos_pair_probe.cpp -- TEST INFRASTRUCTURE, never part of libprt.
//
// sincos_pair of csrc/hip/pt_device.h compiled for the HOST the way tests/emu does it (-DPT_EMU, hipcc --cuda-host-only), next to
// prt_sin / prt_cos of include/prt_detmath.h: tests/test_sincos_pair.py counts the bit patterns on which they differ.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "pt_device.h"

using namespace prt::dev;

namespace {
bool differs(uint32_t bits) {
    const float x = prt_u2f(bits);
    float s, c;
    sincos_pair(x, s, c);
    return prt_f2u(s) != prt_f2u(prt_sin(x)) || prt_f2u(c) != prt_f2u(prt_cos(x));
}
}  // namespace

// the patterns first, first + stride, ... below `end` (64-bit: end = 2^32 is the whole space) on which the helper differs from prt_sin /
// prt_cos in a bit of either result; *first_bad = the lowest of them
extern "C" uint64_t sincos_pair_mismatches(uint64_t first, uint64_t end, uint64_t stride, int threads, uint32_t* first_bad) {
    if (threads < 1) threads = 1;
    const uint64_t count = end > first ? (end - first + stride - 1) / stride : 0;
    std::atomic<uint64_t> bad(0), lowest(~0ull);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) {
        pool.emplace_back([&, t] {
            const uint64_t k0 = count * (uint64_t)t / (uint64_t)threads, k1 = count * (uint64_t)(t + 1) / (uint64_t)threads;
            uint64_t n = 0, low = ~0ull;
            for (uint64_t k = k0; k < k1; ++k) {
                const uint64_t bits = first + k * stride;
                if (differs((uint32_t)bits)) { ++n; if (bits < low) low = bits; }
            }
            bad += n;
            uint64_t cur = lowest.load();
            while (low < cur && !lowest.compare_exchange_weak(cur, low)) {}
        });
    }
    for (auto& th : pool) th.join();
    if (first_bad && bad.load()) *first_bad = (uint32_t)lowest.load();
    return bad.load();
}

// both forms on a caller's vector: pair_s / pair_c from the helper, ref_s / ref_c from prt_sin / prt_cos
extern "C" void sincos_pair_eval(const float* x, float* pair_s, float* pair_c, float* ref_s, float* ref_c, int n) {
    for (int i = 0; i < n; ++i) {
        sincos_pair(x[i], pair_s[i], pair_c[i]);
        ref_s[i] = prt_sin(x[i]);
        ref_c[i] = prt_cos(x[i]);
    }
}
