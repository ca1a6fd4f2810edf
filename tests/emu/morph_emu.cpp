// tests/emu/morph_emu.cpp -- TEST INFRASTRUCTURE: the bodies of the morph kernels (csrc/hip/pt_morph.h) compiled for the host and run serially,
// one corner after the other, and the checks and the table builder of prt_set_morph_targets (the same host functions).
// tests/emu/morph_api.py binds it.  With -DMORPH_EMU_MAIN a stand-alone program for sanitizer runs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prt.h"
#include "pt_morph.h"

using namespace prt;

extern "C" {

// the refusals of prt_set_morph_targets: 0 = accepted, else the code it returns (PRT_ERR_INVALID_ARGUMENT, PRT_ERR_UNSUPPORTED)
int morph_emu_check(const prt_morph_set* set, uint32_t n_tris) {
    int code = 0;
    return morph_set_error(set, n_tris, &code) ? code : 0;
}

// the table of an accepted set: the number of entries; offset (3 n_tris + 1 words) and the records (16 bytes each; entry_n only with base
// normals) are copied out when the pointers are given
uint32_t morph_emu_table(const prt_morph_set* set, uint32_t n_tris, uint32_t* offset, float* entry_p, float* entry_n) {
    MorphTable tab;
    morph_build_table(set, n_tris, tab);
    if (offset) std::memcpy(offset, tab.offset.data(), tab.offset.size() * 4);
    if (entry_p && !tab.entry_p.empty()) std::memcpy(entry_p, tab.entry_p.data(), tab.entry_p.size() * 16);
    if (entry_n && !tab.entry_n.empty()) std::memcpy(entry_n, tab.entry_n.data(), tab.entry_n.size() * 16);
    return (uint32_t)tab.entry_p.size();
}

// what prt_morph does before the refit or the rebuild: out_v and (with base_n) out_n, float4[n_corners] each, every pointer to floats 16-byte
// aligned.  Nothing is checked: the body is run as the kernel runs it
void morph_emu_morph(const float* base_v, const float* base_n, const uint32_t* offset, const float* entry_p, const float* entry_n,
                     const float* weights, uint32_t n_corners, float* out_v, float* out_n) {
    for (size_t c = 0; c < n_corners; ++c) morph_corner(base_v, base_n, offset, entry_p, entry_n, weights, c, out_v, base_n ? out_n : nullptr);
}

// ... and prt_pose_morphed
void morph_emu_pose_morphed(const float* base_v, const float* base_n, const uint32_t* offset, const float* entry_p, const float* entry_n,
                            const float* weights, const uint16_t* bone_index, const float* bone_weight, const float* matrices, uint32_t n_corners,
                            float* out_v, float* out_n) {
    for (size_t c = 0; c < n_corners; ++c)
        pose_morphed_corner(base_v, base_n, offset, entry_p, entry_n, weights, bone_index, bone_weight, matrices, c, out_v, base_n ? out_n : nullptr);
}

uint32_t morph_emu_max_targets() { return PT_MORPH_MAX_TARGETS; }

}  // extern "C"

#ifdef MORPH_EMU_MAIN
// Sanitizer program (development, CPU only; -fsanitize=address,undefined): meshes of 1, 22, 86 and 1031 triangles with exactly-sized sets of
// 1, 3, 257 and 65536 targets and exactly-sized tables -- a record read past a corner's range, a weight read past the table, or a write past
// the table in the builder would be seen.  Checks the planted cases of prt.h against values computed here.
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
    int bad = 0;
    for (uint32_t T : {1u, 22u, 86u, 1031u})
        for (uint32_t nt : {1u, 3u, 257u, 65536u}) {
            const size_t n = 3 * (size_t)T;
            std::vector<RefitQuad> v(n), nr(n), ov(n), on(n);
            for (size_t c = 0; c < n; ++c) {
                v[c] = RefitQuad{0.01f * (float)(c % 97), 1.0f - 0.02f * (float)(c % 31), -0.0f, 7.0f};
                nr[c] = RefitQuad{0.0f, 0.6f, 0.8f, 9.0f};
            }
            // target t lists corner 0 (all of them do), a few corners by a stride of its own, and -- the last target only -- the last corner;
            // target 1 (when there is one) has no entries at all
            std::vector<std::vector<uint32_t>> corner(nt);
            std::vector<std::vector<RefitQuad>> dp(nt), dn(nt);
            std::vector<prt_morph_target> tg(nt);
            std::vector<float> w(nt);                                      // exactly sized: a target number past the table is a heap overflow
            for (uint32_t t = 0; t < nt; ++t) {
                w[t] = t % 3 == 2 ? -0.0f : 0.25f + 0.001f * (float)(t % 100u);
                if (t == 1 && nt > 2) { tg[t] = prt_morph_target{nullptr, nullptr, nullptr, 0u, 0u}; continue; }
                corner[t].push_back(0u);
                const uint32_t stride = 2u + t % 7u;
                for (uint32_t k = 1; k < 5 && nt <= 257u; ++k) {
                    const size_t c = 1 + (size_t)k * stride + t % 3u;
                    if (c + 1 < n && c > corner[t].back()) corner[t].push_back((uint32_t)c);
                }
                if (t == nt - 1 && n > 1) corner[t].push_back((uint32_t)(n - 1));
                for (size_t j = 0; j < corner[t].size(); ++j) {
                    dp[t].push_back(RefitQuad{0.001f * (float)(t % 50u), -0.002f, 0.0005f * (float)j, __builtin_nanf("")});
                    dn[t].push_back(RefitQuad{0.01f, 0.0f, -0.01f, __builtin_nanf("")});
                }
                tg[t] = prt_morph_target{corner[t].data(), &dp[t][0].x, t % 2 ? nullptr : &dn[t][0].x, (uint32_t)corner[t].size(), 0u};
            }
            for (int with_n = 0; with_n < 2; ++with_n) {
                const prt_morph_set set{&v[0].x, with_n ? &nr[0].x : nullptr, tg.data(), nt, 0u};
                bad += morph_emu_check(&set, T) != 0;
                MorphTable tab;
                morph_build_table(&set, T, tab);
                tab.offset.shrink_to_fit(); tab.entry_p.shrink_to_fit(); tab.entry_n.shrink_to_fit();
                uint64_t total = 0;
                for (uint32_t t = 0; t < nt; ++t) total += tg[t].n_entries;
                bad += tab.offset.size() != n + 1 || tab.offset[n] != total || tab.entry_p.size() != total || tab.entry_n.size() != (with_n ? total : 0);
                for (size_t c = 0; c < n; ++c)                             // ascending targets within a corner
                    for (uint32_t e = tab.offset[c] + 1; e < tab.offset[c + 1]; ++e) bad += morph_target_of(tab.entry_p[e - 1]) >= morph_target_of(tab.entry_p[e]);
                const float* en = with_n ? &tab.entry_n.data()->x : nullptr;
                const float* ep = total ? &tab.entry_p.data()->x : nullptr;
                morph_emu_morph(&v[0].x, with_n ? &nr[0].x : nullptr, tab.offset.data(), ep, en, w.data(), (uint32_t)n, &ov[0].x, &on[0].x);
                // corner 0 by hand, in ascending t
                float px = v[0].x;
                for (uint32_t t = 0; t < nt; ++t)
                    if (tg[t].n_entries && w[t] != 0.0f) px = px + w[t] * dp[t][0].x;
                bad += bits(px) != bits(ov[0].x);
                for (size_t c = 0; c < n; ++c) {
                    bad += !(ov[c].x == ov[c].x && ov[c].w == 0.0f);
                    if (tab.offset[c] == tab.offset[c + 1]) bad += !(bits(ov[c].x) == bits(v[c].x) && bits(ov[c].y) == bits(v[c].y) && bits(ov[c].z) == bits(v[c].z));
                    if (with_n) bad += !(on[c].x == on[c].x && on[c].w == 0.0f);
                }
                // the fused body with one identity bone: ((1 * p.x + 0 * p.y) + 0 * p.z) + 0
                std::vector<PoseIndex> idx(n, PoseIndex{{0, 0, 0, 0}});
                std::vector<RefitQuad> bw(n, RefitQuad{1.0f, 0.0f, 0.0f, -0.0f}), fv(n), fn(n);
                const RefitQuad m[3] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
                morph_emu_pose_morphed(&v[0].x, with_n ? &nr[0].x : nullptr, tab.offset.data(), ep, en, w.data(), idx[0].b, &bw[0].x, &m[0].x, (uint32_t)n,
                                       &fv[0].x, &fn[0].x);
                for (size_t c = 0; c < n; ++c) bad += bits(fv[c].x) != bits(((1.0f * ov[c].x + 0.0f * ov[c].y) + 0.0f * ov[c].z) + 0.0f);
            }
            // the refusals
            const prt_morph_set ok{&v[0].x, &nr[0].x, tg.data(), nt, 0u};
            prt_morph_set s = ok;
            s.base_vertices = nullptr; bad += morph_emu_check(&s, T) != PRT_ERR_INVALID_ARGUMENT;
            s = ok; s.targets = nullptr; bad += morph_emu_check(&s, T) != PRT_ERR_INVALID_ARGUMENT;
            s = ok; s.n_targets = 0u; bad += morph_emu_check(&s, T) != PRT_ERR_INVALID_ARGUMENT;
            s = ok; s.n_targets = 65537u; bad += morph_emu_check(&s, T) != PRT_ERR_INVALID_ARGUMENT;
            {
                std::vector<prt_morph_target> b(tg);
                std::vector<uint32_t> cc(corner[0]);
                cc.back() = (uint32_t)n;                                   // a corner >= 3T
                b[0].corner = cc.data();
                s = ok; s.targets = b.data(); bad += morph_emu_check(&s, T) != PRT_ERR_INVALID_ARGUMENT;
                std::vector<RefitQuad> d(dp[0]);
                d.back().y = __builtin_inff();
                b = tg; b[0].d_position = &d[0].x;
                s = ok; s.targets = b.data(); bad += morph_emu_check(&s, T) != PRT_ERR_INVALID_ARGUMENT;
                b = tg; b[0].d_position = nullptr;
                s = ok; s.targets = b.data(); bad += morph_emu_check(&s, T) != PRT_ERR_INVALID_ARGUMENT;
            }
            std::printf("morph_emu_main: T = %u, %u targets: %d mismatches so far\n", T, nt, bad);
        }
    {
        // one triangle, three targets: deltas that cancel the normal to length 0 (corner 0), denormal deltas (corner 1), a weight that
        // overflows a coordinate to inf and is passed on (corner 2), a -0 weight over NaN deltas (target 2, every corner)
        const float nan = __builtin_nanf("");
        RefitQuad v[3] = {{1, 2, 3, 0}, {0, -0.0f, 1e-45f, 0}, {2, 2, 0, 0}}, nr[3] = {{0, 1, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}}, ov[3], on[3];
        uint32_t c0[1] = {0}, c1[2] = {1, 2}, c2[3] = {0, 1, 2};
        RefitQuad d0[1] = {{0.5f, 0, 0, 0}}, n0[1] = {{0, -1, 0, 0}};
        RefitQuad d1[2] = {{1e-42f, 0, 1e-45f, 0}, {3e38f, 0, 0, 0}}, n1[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        RefitQuad d2[3] = {{nan, nan, nan, 0}, {nan, nan, nan, 0}, {nan, nan, nan, 0}};
        prt_morph_target tg[3] = {{c0, &d0[0].x, &n0[0].x, 1, 0}, {c1, &d1[0].x, &n1[0].x, 2, 0}, {c2, &d2[0].x, &d2[0].x, 3, 0}};
        const prt_morph_set set{&v[0].x, &nr[0].x, tg, 3, 0};
        bad += morph_emu_check(&set, 1) != PRT_ERR_INVALID_ARGUMENT;      // (the NaN deltas: refused by the library, run here as the kernel would)
        MorphTable tab;
        morph_build_table(&set, 1, tab);
        const float w[3] = {1.0f, 2.0f, -0.0f};
        morph_emu_morph(&v[0].x, &nr[0].x, tab.offset.data(), &tab.entry_p[0].x, &tab.entry_n[0].x, w, 3u, &ov[0].x, &on[0].x);
        bad += !(ov[0].x == 1.5f && bits(on[0].x) == 0 && bits(on[0].y) == 0 && bits(on[0].z) == 0);
        bad += !(bits(ov[1].x) == bits(0.0f + 2.0f * 1e-42f) && bits(ov[1].y) == bits(-0.0f + 2.0f * 0.0f) && bits(ov[1].z) == bits(1e-45f + 2.0f * 1e-45f));
        bad += !(ov[2].x == __builtin_inff() && ov[2].y == 2.0f && on[2].x == 1.0f);
    }
    std::printf("morph_emu_main: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
