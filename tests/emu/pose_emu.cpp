// tests/emu/pose_emu.cpp -- TEST INFRASTRUCTURE: the body of the pose kernel (csrc/hip/pt_pose.h) compiled for the host and run serially, one
// corner after the other, and the checks of prt_set_skin (the same host function).  tests/emu/pose_api.py binds it.  With -DPOSE_EMU_MAIN a
// stand-alone program for sanitizer runs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prt.h"
#include "pt_pose.h"

using namespace prt;

extern "C" {

// the refusals of prt_set_skin: 0 = accepted, 1 = refused (rest_normals may be null)
int pose_emu_check(const float* rest_v, const float* rest_n, const uint16_t* bone_index, const float* bone_weight, uint32_t n_bones, uint32_t n_tris) {
    return pose_skin_error(rest_v, rest_n, bone_index, bone_weight, n_bones, n_tris) ? 1 : 0;
}

// what a pose does before the refit or the rebuild: out_v and (with rest_n) out_n, float4[n_corners] each, every pointer to floats 16-byte
// aligned.  Nothing is checked: the body is run as the kernel runs it
void pose_emu_pose(const float* rest_v, const float* rest_n, const uint16_t* bone_index, const float* bone_weight, const float* matrices,
                   uint32_t n_corners, float* out_v, float* out_n) {
    for (size_t c = 0; c < n_corners; ++c) pose_corner(rest_v, rest_n, bone_index, bone_weight, matrices, c, out_v, rest_n ? out_n : nullptr);
}

uint32_t pose_emu_max_bones() { return PT_POSE_MAX_BONES; }

}  // extern "C"

#ifdef POSE_EMU_MAIN
// Sanitizer program (development, CPU only; -fsanitize=address,undefined): meshes of 1, 22, 86 and 1031 triangles with exactly-sized
// tables of 1, 4, 257 and 65536 bones -- a matrix read past the table, or one under a zero weight planted at the table's last entry with an
// index that is only valid because it is never read -- would be seen.  Checks the planted cases of prt.h against values computed here.
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
    int bad = 0;
    for (uint32_t T : {1u, 22u, 86u, 1031u})
        for (uint32_t nb : {1u, 4u, 257u, 65536u}) {
            const size_t n = 3 * (size_t)T;
            std::vector<RefitQuad> v(n), nr(n), w(n), ov(n), on(n);
            std::vector<PoseIndex> idx(n);
            std::vector<RefitQuad> m(3 * (size_t)nb);                     // exactly sized: an index past the table is a heap overflow
            for (uint32_t b = 0; b < nb; ++b) {
                const float a = 0.001f * (float)(b % 1000u), cs = __builtin_cosf(a), sn = __builtin_sinf(a);
                m[3 * b] = RefitQuad{cs, 0.0f, sn, 0.25f * (float)(b % 7u)};
                m[3 * b + 1] = RefitQuad{0.0f, 1.0f, 0.0f, -0.5f};
                m[3 * b + 2] = RefitQuad{-sn, 0.0f, cs, 0.125f};
            }
            for (size_t c = 0; c < n; ++c) {
                v[c] = RefitQuad{0.01f * (float)(c % 97), 1.0f - 0.02f * (float)(c % 31), -0.0f, 7.0f};
                nr[c] = RefitQuad{0.0f, 0.6f, 0.8f, 9.0f};
                for (int k = 0; k < 4; ++k) idx[c].b[k] = (uint16_t)((c * 2654435761u + 40503u * (unsigned)k) % nb);
                w[c] = c % 5 == 0 ? RefitQuad{1.0f, 0.0f, 0.0f, 0.0f} : RefitQuad{0.5f, 0.25f, -0.25f, 0.5f};
            }
            // planted: all weights zero (corner 0); a -0 weight beside a NaN matrix (corner 1, bone nb - 1 made NaN when nb > 1)
            w[0] = RefitQuad{0.0f, -0.0f, 0.0f, 0.0f};
            if (nb > 1) {
                m[3 * (nb - 1)].y = __builtin_nanf("");
                for (size_t c = 0; c < n; ++c)
                    for (int k = 0; k < 4; ++k) if (idx[c].b[k] == nb - 1) idx[c].b[k] = 0;
                idx[1].b[1] = (uint16_t)(nb - 1); idx[1].b[0] = 0;
                w[1] = RefitQuad{1.0f, -0.0f, 0.0f, 0.0f};
            }
            bad += pose_emu_check(&v[0].x, &nr[0].x, idx[0].b, &w[0].x, nb, T) != 0;
            pose_emu_pose(&v[0].x, &nr[0].x, idx[0].b, &w[0].x, &m[0].x, (uint32_t)n, &ov[0].x, &on[0].x);
            bad += !(bits(ov[0].x) == 0 && bits(ov[0].y) == 0 && bits(ov[0].z) == 0 && bits(on[0].x) == 0 && bits(on[0].y) == 0 && bits(on[0].z) == 0);
            for (size_t c = 0; c < n; ++c)
                bad += !(ov[c].x == ov[c].x && ov[c].y == ov[c].y && ov[c].z == ov[c].z && ov[c].w == 0.0f && on[c].x == on[c].x && on[c].w == 0.0f);
            if (T > 1 || nb == 1) {                                       // corner 1 (or any rigid corner): one matrix, applied as prt.h writes it
                const size_t c = nb > 1 ? 1 : 5 % n;
                if (w[c].x == 1.0f && w[c].y == 0.0f) {
                    const RefitQuad* q = &m[3 * (size_t)idx[c].b[0]];
                    const float a00 = 0.0f + 1.0f * q[0].x, a01 = 0.0f + 1.0f * q[0].y, a02 = 0.0f + 1.0f * q[0].z, a03 = 0.0f + 1.0f * q[0].w;
                    const float px = ((a00 * v[c].x + a01 * v[c].y) + a02 * v[c].z) + a03;
                    bad += bits(px) != bits(ov[c].x);
                }
            }
            // without normals: out_n is not touched (a null pointer)
            pose_emu_pose(&v[0].x, nullptr, idx[0].b, &w[0].x, &m[0].x, (uint32_t)n, &ov[0].x, nullptr);
            // the refusals
            std::vector<PoseIndex> bi(idx);
            if (nb < 65536u) { bi[n - 1].b[3] = (uint16_t)nb; bad += pose_emu_check(&v[0].x, nullptr, bi[0].b, &w[0].x, nb, T) != 1; }
            std::vector<RefitQuad> bw(w);
            bw[n / 2].z = __builtin_inff();
            bad += pose_emu_check(&v[0].x, nullptr, idx[0].b, &bw[0].x, nb, T) != 1;
            bad += pose_emu_check(&v[0].x, nullptr, idx[0].b, &w[0].x, 0u, T) != 1;
            bad += pose_emu_check(&v[0].x, nullptr, idx[0].b, &w[0].x, 65537u, T) != 1;
            bad += pose_emu_check(nullptr, nullptr, idx[0].b, &w[0].x, nb, T) != 1;
            std::printf("pose_emu_main: T = %u, %u bones: %d mismatches so far\n", T, nb, bad);
        }
    {
        // one triangle, two bones: a normal that blends to length 0 (corner 0), denormal coordinates (corner 1), a matrix that overflows to
        // inf and is passed on (corner 2: the refusal is the finite-vertex check's, downstream)
        RefitQuad m[6] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {3e38f, 3e38f, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
        RefitQuad v[3] = {{1, 2, 3, 0}, {1e-42f, -2e-44f, 1e-45f, 0}, {2, 2, 0, 0}}, nr[3] = {{0, 1, 0, 0}, {1e-42f, 0, 0, 0}, {1, 0, 0, 0}}, ov[3], on[3];
        RefitQuad w[3] = {{0.5f, -0.5f, 0, 0}, {1, 0, 0, 0}, {0, 1, 0, 0}};
        PoseIndex idx[3] = {{{0, 0, 1, 1}}, {{0, 1, 1, 1}}, {{0, 1, 0, 0}}};
        pose_emu_pose(&v[0].x, &nr[0].x, idx[0].b, &w[0].x, &m[0].x, 3u, &ov[0].x, &on[0].x);
        bad += !(bits(on[0].x) == 0 && bits(on[0].y) == 0 && bits(on[0].z) == 0 && bits(ov[0].x) == 0);
        bad += !(bits(ov[1].x) == bits(1e-42f) && bits(ov[1].y) == bits(-2e-44f + 0.0f) && bits(ov[1].z) == bits(1e-45f) && bits(on[1].x) == bits(1e-42f));     // (the normal's square underflows: L == 0 keeps n')
        bad += !(ov[2].x == __builtin_inff() && ov[2].y == 2.0f && bits(on[2].x) == 0);                      // (3e38 / inf)
    }
    std::printf("pose_emu_main: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
