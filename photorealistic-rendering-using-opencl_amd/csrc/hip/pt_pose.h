// pt_pose.h -- the body of the pose kernel (pt_pose.hip; prt.h prt_set_skin / prt_pose): rest pose + per-corner influences + the frame's bone
// matrices -> posed vertices and normals, linear blend skinning written as the formulas of prt.h.  Plain pointers and a __host__ __device__
// inline function only, as pt_refit.h and pt_normals.h, so that a host harness (tests/emu/pose_emu.cpp) runs the same code serially.  f32
// operations in the order of prt.h, no contraction (build.py: -ffp-contract=off); sqrtf and / are the correctly rounded ones on both sides.
// The host-only part below the body: the checks of prt_set_skin.
#pragma once
#include <stdint.h>

#include "pt_refit.h"             // RefitQuad: one 16-byte access

#define PT_POSE_HD PT_REFIT_HD

namespace prt {

// the four bone indices of a corner: one 8-byte access
struct alignas(8) PoseIndex { uint16_t b[4]; };

// The matrix table stays in global memory and is read through the CU's vector cache (32 KiB): 256 bones are 12 KiB and stay there, 65 536
// are 3 MiB and stay in the XCD's L2.  There is no LDS staging and hence no threshold between two kernels: a block of 256 corners would
// copy the table (48 bytes per bone) to read at most 1 024 matrices of it, against 88 streamed bytes per corner (DESIGN.md s4 "Posing").
// Rows of a matrix are 16 bytes: three 16-byte loads per influence
constexpr uint32_t PT_POSE_MAX_BONES = 65536u;

// Corner c: A = +0;  for k = 0 .. 3 with w_k != 0 (a zero of either sign skips the influence and its matrix is not read):
// A_ij = A_ij + w_k * M[b_k]_ij;  p' = ((A_i0 * x + A_i1 * y) + A_i2 * z) + A_i3;  n' = (A_i0 * nx + A_i1 * ny) + A_i2 * nz, L = |n'|,
// normal = L > 0 ? n' / L : n'.  Lane 3 of both outputs = 0.  rest_n null: no normals (out_n is not written)
// As a function of the corner's loaded values (p: the rest position, lane 3 unused; rest_normal(): the rest normal, asked for after the vertex
// has been stored and only with has_n), so that pt_morph.h poses a rest pose that exists in registers only
template <typename RestNormal>
PT_POSE_HD void pose_values(const RefitQuad& p, bool has_n, RestNormal rest_normal, const RefitQuad& wq, const PoseIndex& idx, const float* matrices,
                            size_t c, float* out_v, float* out_n) {
    const float w[4] = {wq.x, wq.y, wq.z, wq.w};
    RefitQuad r0{0.0f, 0.0f, 0.0f, 0.0f}, r1 = r0, r2 = r0;
    for (int k = 0; k < 4; ++k) {
        if (w[k] != 0.0f) {
            const RefitQuad* m = reinterpret_cast<const RefitQuad*>(matrices) + 3 * (size_t)idx.b[k];
            const RefitQuad m0 = m[0], m1 = m[1], m2 = m[2];
            r0.x = r0.x + w[k] * m0.x; r0.y = r0.y + w[k] * m0.y; r0.z = r0.z + w[k] * m0.z; r0.w = r0.w + w[k] * m0.w;
            r1.x = r1.x + w[k] * m1.x; r1.y = r1.y + w[k] * m1.y; r1.z = r1.z + w[k] * m1.z; r1.w = r1.w + w[k] * m1.w;
            r2.x = r2.x + w[k] * m2.x; r2.y = r2.y + w[k] * m2.y; r2.z = r2.z + w[k] * m2.z; r2.w = r2.w + w[k] * m2.w;
        }
    }
    reinterpret_cast<RefitQuad*>(out_v)[c] = RefitQuad{((r0.x * p.x + r0.y * p.y) + r0.z * p.z) + r0.w, ((r1.x * p.x + r1.y * p.y) + r1.z * p.z) + r1.w,
                                                       ((r2.x * p.x + r2.y * p.y) + r2.z * p.z) + r2.w, 0.0f};
    if (has_n) {
        const RefitQuad n = rest_normal();
        const float nx = (r0.x * n.x + r0.y * n.y) + r0.z * n.z;
        const float ny = (r1.x * n.x + r1.y * n.y) + r1.z * n.z;
        const float nz = (r2.x * n.x + r2.y * n.y) + r2.z * n.z;
        const float L = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
        const bool unit = L > 0.0f;
        reinterpret_cast<RefitQuad*>(out_n)[c] = RefitQuad{unit ? nx / L : nx, unit ? ny / L : ny, unit ? nz / L : nz, 0.0f};
    }
}

PT_POSE_HD void pose_corner(const float* rest_v, const float* rest_n, const uint16_t* bone_index, const float* bone_weight, const float* matrices,
                            size_t c, float* out_v, float* out_n) {
    const RefitQuad p = reinterpret_cast<const RefitQuad*>(rest_v)[c];
    const RefitQuad wq = reinterpret_cast<const RefitQuad*>(bone_weight)[c];
    const PoseIndex idx = reinterpret_cast<const PoseIndex*>(bone_index)[c];
    pose_values(p, rest_n != nullptr, [=]() { return reinterpret_cast<const RefitQuad*>(rest_n)[c]; }, wq, idx, matrices, c, out_v, out_n);
}

// ---- host only ----------------------------------------------------------------------------------------------------------------------------------

// the refusals of prt_set_skin over the caller's host arrays (plain reads: they need not be aligned); null = accepted, else what is wrong.
// rest_normals may be null
inline const char* pose_skin_error(const float* rest_vertices, const float* rest_normals, const uint16_t* bone_index, const float* bone_weight,
                                   uint32_t n_bones, uint32_t n_tris) {
    if (!rest_vertices || !bone_index || !bone_weight) return "null rest_vertices, bone_index or bone_weight";
    if (n_bones < 1u || n_bones > PT_POSE_MAX_BONES) return "n_bones outside 1 .. 65536";
    const float fmax = 3.4028234663852886e+38f;
    const size_t n = 3 * (size_t)n_tris;
    for (size_t c = 0; c < n; ++c) {
        for (int k = 0; k < 4; ++k) {
            if (bone_index[4 * c + k] >= n_bones) return "a bone index >= n_bones";
            if (!(__builtin_fabsf(bone_weight[4 * c + k]) <= fmax)) return "a weight that is not finite";
        }
        for (int k = 0; k < 3; ++k) {
            if (!(__builtin_fabsf(rest_vertices[4 * c + k]) <= fmax)) return "a rest vertex with a non-finite x, y or z";
            if (rest_normals && !(__builtin_fabsf(rest_normals[4 * c + k]) <= fmax)) return "a rest normal with a non-finite component";
        }
    }
    return nullptr;
}

}  // namespace prt
