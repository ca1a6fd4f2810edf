// tests/emu/motion_emu.cpp -- TEST INFRASTRUCTURE: the bodies of the motion plane (csrc/hip/pt_motion.h) compiled for the host, as
// refit_emu.cpp does for the refit.  tests/emu/motion_api.py binds it.  With -DMOTION_EMU_MAIN a stand-alone program for sanitizer runs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pt_motion.h"

using namespace prt;

extern "C" {

// case i: d = motion_displacement(prev, cur, slots[i], uv[2 i], uv[2 i + 1]); prev / cur: n_slots records of 12 floats (16-byte aligned)
void motion_emu_displacement(const void* prev, const void* cur, const uint32_t* slots, const float* uv, uint32_t n, float* out3) {
    const TriGeom* p = static_cast<const TriGeom*>(prev);
    const TriGeom* c = static_cast<const TriGeom*>(cur);
    for (uint32_t i = 0; i < n; ++i) {
        const MotionVec d = motion_displacement(p, c, slots[i], uv[2 * i], uv[2 * i + 1]);
        out3[3 * i] = d.x; out3[3 * i + 1] = d.y; out3[3 * i + 2] = d.z;
    }
}

// one pixel: K samples in order; hit[s] counts into the guides' hits, contributing[s] (a direct triangle hit) adds d3[3 s ..] to the sum
void motion_emu_pixel(const float* d3, const uint8_t* hit, const uint8_t* contributing, uint32_t K, float* out4) {
    MotionSum s = motion_sum_begin();
    uint32_t hits = 0;
    for (uint32_t k = 0; k < K; ++k) {
        if (!hit[k]) continue;
        ++hits;
        if (contributing[k]) motion_sum_add(s, MotionVec{d3[3 * k], d3[3 * k + 1], d3[3 * k + 2]});
    }
    const MotionQuad m = motion_pixel(s, hits, K);
    out4[0] = m.x; out4[1] = m.y; out4[2] = m.z; out4[3] = m.w;
}

}  // extern "C"

#ifdef MOTION_EMU_MAIN
// Sanitizer program (development, CPU only): build with -fsanitize=address,undefined and run; exercises both bodies on a few records.
int main() {
    std::vector<TriGeom> prev(5), cur(5);
    for (size_t s = 0; s < prev.size(); ++s)
        for (int k = 0; k < 3; ++k) {
            prev[s].p0[k] = 0.25f * (float)(s + k); prev[s].e1[k] = 1.0f + (float)k; prev[s].e2[k] = 0.5f - (float)s; prev[s].n[k] = 0.0f;
        }
    for (size_t s = 0; s < prev.size(); ++s) {
        cur[s] = prev[s];
        for (int k = 0; k < 3; ++k) cur[s].p0[k] += 0.125f * (float)(k + 1);
    }
    const uint32_t slots[4] = {0, 4, 2, 4};
    const float uv[8] = {0.0f, 0.0f, 0.25f, 0.5f, 1.0f, 0.0f, 0.25f, 0.75f};
    float d[12], px[4];
    motion_emu_displacement(prev.data(), cur.data(), slots, uv, 4, d);
    const uint8_t hit[4] = {1, 1, 0, 1}, con[4] = {1, 0, 0, 1};
    motion_emu_pixel(d, hit, con, 4, px);
    int bad = 0;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 3; ++k) bad += d[3 * i + k] != -0.125f * (float)(k + 1);
    bad += px[3] != 0.5f;
    bad += px[0] != (d[0] + d[9]) / 3.0f;
    std::printf("motion_emu_main: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
