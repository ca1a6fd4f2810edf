// tests/emu/morph_planes_emu.cpp -- TEST INFRASTRUCTURE: the bodies of the plane-layout morph kernels (csrc/hip/pt_morph.h
// morph_planes_corner / pose_morphed_planes_corner) compiled for the host and run serially, one (block, lane) after the other in the
// kernel's launch shape, and the builder of the plane table and the report's arithmetic (the same host functions).
// tests/emu/morph_planes_api.py binds it.  With -DMORPH_PLANES_EMU_MAIN a stand-alone program for sanitizer runs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prt.h"
#include "pt_morph.h"

using namespace prt;

extern "C" {

// the plane table of an accepted set: out4 = {planes, entries}; block_first (ceil(3 n_tris / 64) + 1 words), the heads (16 bytes each) and
// the rows (768 bytes per plane; plane_n only with base normals) are copied out when the pointers are given
void morph_planes_emu_table(const prt_morph_set* set, uint32_t n_tris, uint64_t* counts, uint32_t* block_first, uint32_t* head, float* plane_p,
                            float* plane_n) {
    MorphPlanes pl;
    morph_build_planes(set, n_tris, pl);
    counts[0] = pl.head.size();
    counts[1] = pl.entries;
    if (block_first) std::memcpy(block_first, pl.block_first.data(), pl.block_first.size() * 4);
    if (head && !pl.head.empty()) std::memcpy(head, pl.head.data(), pl.head.size() * 16);
    if (plane_p && !pl.plane_p.empty()) std::memcpy(plane_p, pl.plane_p.data(), pl.plane_p.size() * 4);
    if (plane_n && !pl.plane_n.empty()) std::memcpy(plane_n, pl.plane_n.data(), pl.plane_n.size() * 4);
}

// prt_get_morph_report's table_bytes
uint64_t morph_planes_emu_table_bytes(uint32_t layout, uint32_t n_tris, uint64_t entries, uint64_t planes, int with_normals) {
    return morph_table_bytes(layout, n_tris, entries, planes, with_normals != 0);
}

// what prt_morph does before the refit or the rebuild, in the launch shape of morph_planes_kernel: workgroups of four blocks, lanes past
// n_corners leave.  Nothing is checked: the body is run as the kernel runs it
void morph_planes_emu_morph(const float* base_v, const float* base_n, const uint32_t* block_first, const uint32_t* head, const float* plane_p,
                            const float* plane_n, const float* weights, uint32_t n_corners, float* out_v, float* out_n) {
    const uint32_t groups = (n_corners + 255u) / 256u;
    for (uint32_t g = 0; g < groups; ++g)
        for (uint32_t tid = 0; tid < 256u; ++tid) {
            const uint32_t b = g * 4u + (tid >> 6), l = tid & 63u;
            if ((size_t)b * 64 + l >= n_corners) continue;
            morph_planes_corner(base_v, base_n, block_first, reinterpret_cast<const MorphPlaneHead*>(head), plane_p, plane_n, weights, b, l, out_v,
                                base_n ? out_n : nullptr);
        }
}

// ... and prt_pose_morphed
void morph_planes_emu_pose_morphed(const float* base_v, const float* base_n, const uint32_t* block_first, const uint32_t* head, const float* plane_p,
                                   const float* plane_n, const float* weights, const uint16_t* bone_index, const float* bone_weight,
                                   const float* matrices, uint32_t n_corners, float* out_v, float* out_n) {
    const uint32_t groups = (n_corners + 255u) / 256u;
    for (uint32_t g = 0; g < groups; ++g)
        for (uint32_t tid = 0; tid < 256u; ++tid) {
            const uint32_t b = g * 4u + (tid >> 6), l = tid & 63u;
            if ((size_t)b * 64 + l >= n_corners) continue;
            pose_morphed_planes_corner(base_v, base_n, block_first, reinterpret_cast<const MorphPlaneHead*>(head), plane_p, plane_n, weights, bone_index,
                                       bone_weight, matrices, b, l, out_v, base_n ? out_n : nullptr);
        }
}

}  // extern "C"

#ifdef MORPH_PLANES_EMU_MAIN
// Sanitizer program (development, CPU only; -fsanitize=address,undefined): meshes of 1, 22, 64, 86 and 1031 triangles with exactly-sized sets
// of 1, 3, 257 and 65536 targets and exactly-sized tables -- a row read past the table, a weight read past its table or a write past a
// plane in the builder would be seen -- and every result compared, bit for bit, with the per-corner body over the per-corner table.
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
    int bad = 0;
    for (uint32_t T : {1u, 22u, 64u, 86u, 1031u})
        for (uint32_t nt : {1u, 3u, 257u, 65536u}) {
            const size_t n = 3 * (size_t)T;
            std::vector<RefitQuad> v(n), nr(n), ov(n), on(n), cv(n), cn(n);
            for (size_t c = 0; c < n; ++c) {
                v[c] = RefitQuad{0.01f * (float)(c % 97), 1.0f - 0.02f * (float)(c % 31), -0.0f, 7.0f};
                nr[c] = RefitQuad{0.0f, 0.6f, 0.8f, 9.0f};
            }
            // target 0 is dense; target t lists corner 0, a few corners by a stride of its own and -- the last target only -- the last corner;
            // target 1 (when there is one) has no entries
            std::vector<std::vector<uint32_t>> corner(nt);
            std::vector<std::vector<RefitQuad>> dp(nt), dn(nt);
            std::vector<prt_morph_target> tg(nt);
            std::vector<float> w(nt);
            for (uint32_t t = 0; t < nt; ++t) {
                w[t] = t % 3 == 2 ? -0.0f : 0.25f + 0.001f * (float)(t % 100u);
                if (t == 1 && nt > 2) { tg[t] = prt_morph_target{nullptr, nullptr, nullptr, 0u, 0u}; continue; }
                if (t == 0) {
                    for (size_t c = 0; c < n; ++c) corner[t].push_back((uint32_t)c);
                } else {
                    corner[t].push_back(0u);
                    const uint32_t stride = 29u + t % 7u;
                    for (uint32_t k = 1; k < 5 && nt <= 257u; ++k) {
                        const size_t c = 1 + (size_t)k * stride + t % 3u;
                        if (c + 1 < n && c > corner[t].back()) corner[t].push_back((uint32_t)c);
                    }
                    if (t == nt - 1 && n > 1) corner[t].push_back((uint32_t)(n - 1));
                }
                for (size_t j = 0; j < corner[t].size(); ++j) {
                    dp[t].push_back(RefitQuad{0.001f * (float)(t % 50u), -0.002f, 0.0005f * (float)(j % 64), __builtin_nanf("")});
                    dn[t].push_back(RefitQuad{0.01f, 0.0f, -0.01f, __builtin_nanf("")});
                }
                tg[t] = prt_morph_target{corner[t].data(), &dp[t][0].x, t % 2 ? nullptr : &dn[t][0].x, (uint32_t)corner[t].size(), 0u};
            }
            for (int with_n = 0; with_n < 2; ++with_n) {
                const prt_morph_set set{&v[0].x, with_n ? &nr[0].x : nullptr, tg.data(), nt, 0u};
                int code = 0;
                bad += morph_set_error(&set, T, &code) != nullptr;
                MorphPlanes pl;
                morph_build_planes(&set, T, pl);
                pl.block_first.shrink_to_fit(); pl.head.shrink_to_fit(); pl.plane_p.shrink_to_fit(); pl.plane_n.shrink_to_fit();
                const size_t blocks = (n + 63) / 64, P = pl.head.size();
                bad += pl.block_first.size() != blocks + 1 || pl.block_first[blocks] != P || pl.plane_p.size() != 192 * P ||
                       pl.plane_n.size() != (with_n ? 192 * P : 0);
                uint64_t listed = 0;
                for (size_t b = 0; b < blocks; ++b)
                    for (uint32_t u = pl.block_first[b]; u < pl.block_first[b + 1]; ++u) {
                        if (u > pl.block_first[b]) bad += pl.head[u - 1].target >= pl.head[u].target;             // ascending targets within a block
                        const uint64_t mask = (uint64_t)pl.head[u].mask_hi << 32 | pl.head[u].mask_lo;
                        bad += mask == 0 || pl.head[u].zero != 0;
                        listed += (uint64_t)__builtin_popcountll(mask);
                        for (uint32_t l = 0; l < 64; ++l) bad += ((mask >> l) & 1u) && b * 64 + l >= n;            // no lane past 3T
                    }
                bad += listed != pl.entries;
                MorphTable tab;
                morph_build_table(&set, T, tab);
                const float* en = with_n ? &tab.entry_n.data()->x : nullptr;
                for (size_t c = 0; c < n; ++c) morph_corner(&v[0].x, with_n ? &nr[0].x : nullptr, tab.offset.data(), &tab.entry_p.data()->x, en, w.data(), c,
                                                            &cv[0].x, with_n ? &cn[0].x : nullptr);
                morph_planes_emu_morph(&v[0].x, with_n ? &nr[0].x : nullptr, pl.block_first.data(), &pl.head.data()->target, pl.plane_p.data(),
                                       with_n ? pl.plane_n.data() : nullptr, w.data(), (uint32_t)n, &ov[0].x, &on[0].x);
                for (size_t c = 0; c < n; ++c) {
                    bad += !(bits(ov[c].x) == bits(cv[c].x) && bits(ov[c].y) == bits(cv[c].y) && bits(ov[c].z) == bits(cv[c].z) && bits(ov[c].w) == 0);
                    if (with_n) bad += !(bits(on[c].x) == bits(cn[c].x) && bits(on[c].y) == bits(cn[c].y) && bits(on[c].z) == bits(cn[c].z) && bits(on[c].w) == 0);
                }
                // the fused body with one identity bone against the per-corner fused body
                std::vector<PoseIndex> idx(n, PoseIndex{{0, 0, 0, 0}});
                std::vector<RefitQuad> bw(n, RefitQuad{1.0f, 0.0f, 0.0f, -0.0f}), fv(n), fn(n), gv(n), gn(n);
                const RefitQuad m[3] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
                morph_planes_emu_pose_morphed(&v[0].x, with_n ? &nr[0].x : nullptr, pl.block_first.data(), &pl.head.data()->target, pl.plane_p.data(),
                                              with_n ? pl.plane_n.data() : nullptr, w.data(), idx[0].b, &bw[0].x, &m[0].x, (uint32_t)n, &fv[0].x, &fn[0].x);
                for (size_t c = 0; c < n; ++c)
                    pose_morphed_corner(&v[0].x, with_n ? &nr[0].x : nullptr, tab.offset.data(), &tab.entry_p.data()->x, en, w.data(), idx[0].b, &bw[0].x,
                                        &m[0].x, c, &gv[0].x, with_n ? &gn[0].x : nullptr);
                for (size_t c = 0; c < n; ++c) {
                    bad += std::memcmp(&fv[c], &gv[c], 16) != 0;
                    if (with_n) bad += std::memcmp(&fn[c], &gn[c], 16) != 0;
                }
            }
            std::printf("morph_planes_emu_main: T = %u, %u targets: %d mismatches so far\n", T, nt, bad);
        }
    std::printf("morph_planes_emu_main: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
