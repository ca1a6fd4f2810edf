// tests/emu/normals_emu.cpp -- TEST INFRASTRUCTURE: the bodies of the smooth-normal kernels (csrc/hip/pt_normals.h) compiled for the host and run
// serially in the order the device's two launches impose (every face, then every corner), over the group table prt_set_smooth_normals
// builds (the same host function).  tests/emu/normals_api.py binds it.  With -DNORMALS_EMU_MAIN a stand-alone program for sanitizer runs.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "prt.h"
#include "pt_normals.h"

using namespace prt;

extern "C" {

// the weld of prt_weld_corners; 0 = ok, 1 = a non-finite vertex
int normals_emu_weld(const float* vertices, uint32_t n_tris, uint32_t* corner_group, uint32_t* n_groups) {
    return normals_weld(vertices, n_tris, corner_group, n_groups) ? 0 : 1;
}

// the group table: group_first [n_groups + 1], member_face [3 n_tris]; 0 = ok, 1 = an id >= n_groups
int normals_emu_table(const uint32_t* corner_group, uint32_t n_tris, uint32_t n_groups, uint32_t* group_first, uint32_t* member_face) {
    std::vector<uint32_t> first, member;
    if (!normals_group_table(corner_group, n_tris, n_groups, first, member)) return 1;
    for (size_t i = 0; i < first.size(); ++i) group_first[i] = first[i];
    for (size_t i = 0; i < member.size(); ++i) member_face[i] = member[i];
    return 0;
}

// what a generation does: normals float4[3 n_tris] (16-byte aligned); face_out (may be null) receives the {f, l} records, n_tris x 4 floats
int normals_emu_generate(const float* vertices, uint32_t n_tris, const uint32_t* corner_group, uint32_t n_groups, uint32_t weighting, float crease_cos,
                         float* normals, float* face_out) {
    std::vector<uint32_t> first, member;
    if (!normals_group_table(corner_group, n_tris, n_groups, first, member)) return 1;
    std::vector<RefitQuad> face_f(n_tris), face_r(weighting == PRT_NORMALS_AREA ? n_tris : 0);
    RefitQuad* fr = weighting == PRT_NORMALS_AREA ? face_r.data() : nullptr;
    for (size_t i = 0; i < n_tris; ++i) normals_face(vertices, i, face_f.data(), fr);
    for (uint32_t c = 0; c < 3u * n_tris; ++c) normals_corner(corner_group, first.data(), member.data(), face_f.data(), fr, crease_cos, c, normals);
    if (face_out)
        for (size_t i = 0; i < n_tris; ++i) { face_out[4 * i] = face_f[i].x; face_out[4 * i + 1] = face_f[i].y; face_out[4 * i + 2] = face_f[i].z; face_out[4 * i + 3] = face_f[i].w; }
    return 0;
}

}  // extern "C"

#ifdef NORMALS_EMU_MAIN
// Sanitizer program (development, CPU only; -fsanitize=address,undefined): a closed fan, a soup with repeated positions and zero-area faces
// through the weld, the table and both weightings; checks that every normal is finite and that the table is a permutation.
int main() {
    int bad = 0;
    for (uint32_t T : {1u, 2u, 300u, 1031u}) {
        std::vector<RefitQuad> v(3 * (size_t)T), n(3 * (size_t)T);
        for (uint32_t i = 0; i < T; ++i) {
            const float a0 = 0.02094395f * (float)i, a1 = 0.02094395f * (float)(i + 1);
            v[3 * i] = RefitQuad{0.0f, 1.0f, -0.0f, 0.0f};
            v[3 * i + 1] = RefitQuad{__builtin_cosf(a0), 0.0f, __builtin_sinf(a0), 0.0f};
            v[3 * i + 2] = i % 7 == 3 ? v[3 * i + 1] : RefitQuad{__builtin_cosf(a1), 0.0f, __builtin_sinf(a1), 0.0f};
        }
        std::vector<uint32_t> g(3 * (size_t)T);
        uint32_t ng = 0;
        bad += normals_emu_weld(&v[0].x, T, g.data(), &ng) != 0;
        std::vector<uint32_t> first(ng + 4u), member(3 * (size_t)T);
        bad += normals_emu_table(g.data(), T, ng + 3u, first.data(), member.data()) != 0;
        bad += first[ng] != 3u * T || first[ng + 3u] != 3u * T;
        for (uint32_t w : {PRT_NORMALS_UNIT, PRT_NORMALS_AREA}) {
            bad += normals_emu_generate(&v[0].x, T, g.data(), ng, w, PRT_LOADER_CREASE_COS, &n[0].x, nullptr) != 0;
            for (const RefitQuad& q : n) bad += !(q.x == q.x && q.y == q.y && q.z == q.z && q.w == 0.0f);
        }
        g[0] = ng;
        bad += normals_emu_generate(&v[0].x, T, g.data(), ng, 0u, 0.0f, &n[0].x, nullptr) != 1;
        std::printf("normals_emu_main: T = %u, %u groups\n", T, ng);
    }
    std::printf("normals_emu_main: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
