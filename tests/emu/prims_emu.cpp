// tests/emu/prims_emu.cpp -- TEST INFRASTRUCTURE: the bodies of prt_update_primitives and of the primitives' motion (csrc/hip/pt_prims.h)
// compiled for the host, as motion_emu.cpp does for the triangles' motion.  tests/emu/prims_api.py binds it.  With -DPRIMS_EMU_MAIN a
// stand-alone program for sanitizer runs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "prt_types.h"
#include "pt_prims.h"

using namespace prt;

extern "C" {

// record i of the `count` prt_mesh records (16-byte aligned; n_spheres spheres, then n_sdfs SDF primitives, then quads) through prims_pack
// into the three tables (16-byte aligned, sized by the counts); bad[i] = the body's return value.  Returns the number of refused records
uint32_t prims_emu_pack(const void* meshes, uint32_t count, uint32_t n_spheres, uint32_t n_sdfs, const uint8_t* types, void* spheres, void* sdfs,
                        void* quads, uint8_t* bad) {
    uint32_t n_bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const bool b = prims_pack(meshes, i, n_spheres, n_sdfs, types, static_cast<DevSphere*>(spheres), static_cast<DevSdf*>(sdfs),
                                  static_cast<DevQuad*>(quads));
        if (bad) bad[i] = b ? 1 : 0;
        n_bad += b ? 1u : 0u;
    }
    return n_bad;
}

// case i: the displacement of hit point p3[3 i ..] on record idx[i]; prev / cur: tables of 16-byte aligned records
void prims_emu_sphere(const void* prev, const void* cur, const uint32_t* idx, const float* p3, uint32_t n, float* out3) {
    for (uint32_t i = 0; i < n; ++i) {
        const MotionVec d = prims_sphere_displacement(static_cast<const DevSphere*>(prev), static_cast<const DevSphere*>(cur), idx[i], p3[3 * i],
                                                      p3[3 * i + 1], p3[3 * i + 2]);
        out3[3 * i] = d.x; out3[3 * i + 1] = d.y; out3[3 * i + 2] = d.z;
    }
}
void prims_emu_quad(const void* prev, const void* cur, const uint32_t* idx, const float* p3, uint32_t n, float* out3) {
    for (uint32_t i = 0; i < n; ++i) {
        const MotionVec d = prims_quad_displacement(static_cast<const DevQuad*>(prev), static_cast<const DevQuad*>(cur), idx[i], p3[3 * i],
                                                    p3[3 * i + 1], p3[3 * i + 2]);
        out3[3 * i] = d.x; out3[3 * i + 1] = d.y; out3[3 * i + 2] = d.z;
    }
}
void prims_emu_sdf(const void* prev, const void* cur, const uint32_t* idx, uint32_t n, float* out3) {
    for (uint32_t i = 0; i < n; ++i) {
        const MotionVec d = prims_sdf_displacement(static_cast<const DevSdf*>(prev), static_cast<const DevSdf*>(cur), idx[i]);
        out3[3 * i] = d.x; out3[3 * i + 1] = d.y; out3[3 * i + 2] = d.z;
    }
}

// one pixel of a scene of n_spheres spheres, n_sdfs SDF primitives and quads behind them, through prims_displacement and the reduction of
// pt_motion.h: sample s hit mesh mid[s] (-2: a miss, -1: a triangle, which contributes tri_d3[3 s ..] when tri_snap is set) at p3[3 s ..];
// first[s]: no delta event before the hit.  prim_snap: a primitive snapshot is pending
void prims_emu_pixel(const void* sph_prev, const void* sph_cur, const void* sdf_prev, const void* sdf_cur, const void* quad_prev, const void* quad_cur,
                     uint32_t n_spheres, uint32_t n_sdfs, const int32_t* mid, const uint8_t* first, const float* p3, const float* tri_d3,
                     int tri_snap, int prim_snap, uint32_t K, float* out4) {
    const PrimPrev prev{static_cast<const DevSphere*>(sph_prev), static_cast<const DevSdf*>(sdf_prev), static_cast<const DevQuad*>(quad_prev)};
    MotionSum s = motion_sum_begin();
    uint32_t hits = 0;
    for (uint32_t k = 0; k < K; ++k) {
        if (mid[k] < -1) continue;
        ++hits;
        if (!first[k]) continue;
        if (mid[k] == -1) {
            if (tri_snap) motion_sum_add(s, MotionVec{tri_d3[3 * k], tri_d3[3 * k + 1], tri_d3[3 * k + 2]});
        } else if (prim_snap) {
            motion_sum_add(s, prims_displacement(prev, static_cast<const DevSphere*>(sph_cur), static_cast<const DevSdf*>(sdf_cur),
                                                 static_cast<const DevQuad*>(quad_cur), n_spheres, n_sdfs, n_spheres + n_sdfs, (uint32_t)mid[k],
                                                 p3[3 * k], p3[3 * k + 1], p3[3 * k + 2]));
        }
    }
    const MotionQuad m = motion_pixel(s, hits, K);
    out4[0] = m.x; out4[1] = m.y; out4[2] = m.z; out4[3] = m.w;
}

}  // extern "C"

#ifdef PRIMS_EMU_MAIN
// Sanitizer program (development, CPU only): build with -fsanitize=address,undefined and run.  Random records of each kind, the edge cases
// (a quad with a zero edge, e0e0 outside [2^-40, 2^40], -0.0 components, a zero radius) and every refusal through the bodies, against
// pack_quad and the plain expressions.
static uint32_t rng_state = 12345u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) * (1.0f / 16777216.0f) * 4.0f - 2.0f; }

int main() {
    const uint32_t n_sph = 301, n_sdf = 203, n_quad = 407, count = n_sph + n_sdf + n_quad;
    std::vector<prt_mesh> meshes(count);
    std::vector<uint8_t> types(count);
    static_assert(sizeof(prt_mesh) == 256, "prt_mesh");
    for (uint32_t i = 0; i < count; ++i) {
        prt_mesh& m = meshes[i];
        std::memset(&m, 0xFF, sizeof(m));                  // (NaN bit patterns in everything that is not read)
        for (int k = 0; k < 3; ++k) m.pos[k] = rnd();
        for (int k = 0; k < 13; ++k) m.joker[k] = rnd();
        m.t = i < n_sph ? 1 : (i < n_sph + n_sdf ? (uint8_t)(4 | (16u << (i & 3))) : 8);
        types[i] = m.t;
    }
    meshes[0].joker[0] = 0.0f;                                                        // a zero radius
    meshes[1].pos[0] = -0.0f;
    prt_mesh& qz = meshes[n_sph + n_sdf];                                             // a zero edge: u0 is NaN
    qz.joker[3] = qz.joker[4] = qz.joker[5] = 0.0f;
    prt_mesh& qs = meshes[n_sph + n_sdf + 1];                                         // e0e0 below 2^-40, e1e1 above 2^40
    qs.joker[3] = 1e-7f; qs.joker[4] = 0.0f; qs.joker[5] = -0.0f; qs.joker[6] = 3e6f;
    std::vector<DevSphere> sph(n_sph);
    std::vector<DevSdf> sdf(n_sdf);
    std::vector<DevQuad> quad(n_quad);
    std::vector<uint8_t> bad(count);
    int wrong = 0;
    wrong += prims_emu_pack(meshes.data(), count, n_sph, n_sdf, types.data(), sph.data(), sdf.data(), quad.data(), bad.data()) != 0;
    for (uint32_t i = 0; i < n_sph; ++i) wrong += std::memcmp(sph[i].pos, meshes[i].pos, 12) != 0 || std::memcmp(&sph[i].radius, meshes[i].joker, 4) != 0;
    for (uint32_t i = 0; i < n_sdf; ++i) {
        const prt_mesh& m = meshes[n_sph + i];
        wrong += std::memcmp(sdf[i].pos, m.pos, 12) != 0 || sdf[i].type != m.t || std::memcmp(sdf[i].params, m.joker, 16) != 0;
    }
    for (uint32_t i = 0; i < n_quad; ++i) {
        DevQuad d;
        std::memset(&d, 0, sizeof(d));
        pack_quad(meshes[n_sph + n_sdf + i].joker, d);
        wrong += std::memcmp(&d, &quad[i], sizeof(d)) != 0;
    }
    wrong += !(quad[0].u0 != quad[0].u0) || !(quad[1].u0 != quad[1].u0) || !(quad[1].u1 != quad[1].u1);
    // the refusals: one record of each kind, every field that is read, NaN and inf; a changed t; and the fields that are not read
    const float nonfinite[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    const uint32_t probe[3] = {5, n_sph + 5, n_sph + n_sdf + 5};
    const int n_joker_read[3] = {1, 4, 13};
    for (int kind = 0; kind < 3; ++kind)
        for (float v : nonfinite) {
            for (int f = 0; f < 3 + n_joker_read[kind]; ++f) {
                if (kind == 2 && f < 3) continue;                                    // (a quad's pos is not read)
                std::vector<prt_mesh> m2 = meshes;
                if (f < 3) m2[probe[kind]].pos[f] = v; else m2[probe[kind]].joker[f - 3] = v;
                wrong += prims_emu_pack(m2.data(), count, n_sph, n_sdf, types.data(), sph.data(), sdf.data(), quad.data(), bad.data()) != 1 || !bad[probe[kind]];
            }
            std::vector<prt_mesh> m3 = meshes;
            m3[probe[kind]].pos[3] = v;
            for (int f = n_joker_read[kind]; f < 16; ++f) m3[probe[kind]].joker[f] = v;
            if (kind == 2) for (int f = 0; f < 3; ++f) m3[probe[kind]].pos[f] = v;
            wrong += prims_emu_pack(m3.data(), count, n_sph, n_sdf, types.data(), sph.data(), sdf.data(), quad.data(), bad.data()) != 0;
        }
    for (int kind = 0; kind < 3; ++kind) {
        std::vector<prt_mesh> m2 = meshes;
        m2[probe[kind]].t ^= 32;
        wrong += prims_emu_pack(m2.data(), count, n_sph, n_sdf, types.data(), sph.data(), sdf.data(), quad.data(), bad.data()) != 1;
    }
    // the displacements: an unchanged table gives +0, a translated one the translation
    prims_emu_pack(meshes.data(), count, n_sph, n_sdf, types.data(), sph.data(), sdf.data(), quad.data(), nullptr);
    std::vector<DevSphere> sph2 = sph;
    std::vector<DevQuad> quad2 = quad;
    std::vector<DevSdf> sdf2 = sdf;
    for (auto& s : sph2) s.pos[1] += 0.25f;
    for (auto& s : sdf2) s.pos[2] -= 0.5f;
    for (uint32_t i = 2; i < n_sph; ++i) {
        const uint32_t idx = i;
        const float p[3] = {sph[i].pos[0] + sph[i].radius, sph[i].pos[1], sph[i].pos[2]};
        float d[3];
        prims_emu_sphere(sph.data(), sph.data(), &idx, p, 1, d);
        uint32_t bits[3];
        std::memcpy(bits, d, 12);
        if (sph[i].radius != 0.0f) wrong += (bits[0] | bits[1] | bits[2]) != 0;
    }
    for (uint32_t i = 2; i < n_quad; ++i) {
        const uint32_t idx = i;
        const float p[3] = {quad[i].anchor[0] + 0.25f * quad[i].edge0[0], quad[i].anchor[1] + 0.25f * quad[i].edge0[1], quad[i].anchor[2] + 0.25f * quad[i].edge0[2]};
        float d[3];
        prims_emu_quad(quad.data(), quad2.data(), &idx, p, 1, d);
        uint32_t bits[3];
        std::memcpy(bits, d, 12);
        wrong += (bits[0] | bits[1] | bits[2]) != 0;
    }
    for (uint32_t i = 0; i < n_sdf; ++i) {
        const uint32_t idx = i;
        float d[3];
        prims_emu_sdf(sdf.data(), sdf2.data(), &idx, 1, d);
        wrong += d[0] != 0.0f || d[1] != 0.0f || d[2] != sdf[i].pos[2] - sdf2[i].pos[2];
    }
    // the reduction over mixed kinds and misses
    const int32_t mid[6] = {-2, -1, 3, (int32_t)n_sph + 2, (int32_t)(n_sph + n_sdf) + 4, 7};
    const uint8_t first[6] = {1, 1, 1, 1, 1, 0};
    float p3[18], tri[18], px[4];
    for (int k = 0; k < 18; ++k) { p3[k] = rnd(); tri[k] = 0.125f; }
    prims_emu_pixel(sph.data(), sph2.data(), sdf.data(), sdf2.data(), quad.data(), quad2.data(), n_sph, n_sdf, mid, first, p3, tri, 1, 1, 6, px);
    wrong += px[3] != 4.0f * (1.0f / 6.0f);
    prims_emu_pixel(sph.data(), sph2.data(), sdf.data(), sdf2.data(), quad.data(), quad2.data(), n_sph, n_sdf, mid, first, p3, tri, 0, 1, 6, px);
    wrong += px[3] != 3.0f * (1.0f / 6.0f);
    prims_emu_pixel(sph.data(), sph2.data(), sdf.data(), sdf2.data(), quad.data(), quad2.data(), n_sph, n_sdf, mid, first, p3, tri, 1, 0, 6, px);
    wrong += px[3] != 1.0f * (1.0f / 6.0f) || px[0] != 0.125f / 5.0f;
    std::printf("prims_emu_main: %d mismatches\n", wrong);
    return wrong ? 1 : 0;
}
#endif
