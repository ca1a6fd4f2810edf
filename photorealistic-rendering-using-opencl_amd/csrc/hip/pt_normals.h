// pt_normals.h -- the bodies of the smooth-normal kernels (pt_normals.hip; prt.h prt_set_smooth_normals): new vertices -> one face record per
// triangle -> one shading normal per corner, by the loader's rule (csrc/host/model_loader.cpp smooth_missing_normals) written as the formulas
// of prt.h.  Plain pointers and __host__ __device__ inline functions only, as pt_refit.h, so that a host harness (tests/emu/normals_emu.cpp)
// runs the same code serially.  f32 operations in the order of prt.h, no contraction (build.py: -ffp-contract=off); sqrtf and / are the
// correctly rounded ones on both sides.  The host-only part below the bodies: the weld and the group-to-members table.
#pragma once
#include <stdint.h>

#include <cstring>
#include <unordered_map>
#include <vector>

#include "pt_refit.h"             // RefitQuad: one 16-byte access

#define PT_NRM_HD PT_REFIT_HD

namespace prt {

// Face i: a = v[3i], b = v[3i + 1], c = v[3i + 2];  r = cross(b - a, c - a), l = |r|, f = l > 0 ? r / l : r (unit_face_normal of the loader;
// the opposite way from TriGeom's n, and not derived from it: the signs of zeros would differ).  face_f[i] = {f, l}: what a corner gathers
// per member, one 16-byte record; face_r[i] = {r, 0} only for the area weighting (null otherwise)
PT_NRM_HD void normals_face(const float* vertices, size_t i, RefitQuad* face_f, RefitQuad* face_r) {
    const RefitQuad* v = reinterpret_cast<const RefitQuad*>(vertices) + 3 * i;
    const RefitQuad a = v[0], b = v[1], c = v[2];
    const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
    const float wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
    const float rx = uy * wz - uz * wy;
    const float ry = uz * wx - ux * wz;
    const float rz = ux * wy - uy * wx;
    const float l = __builtin_sqrtf((rx * rx + ry * ry) + rz * rz);
    const bool unit = l > 0.0f;
    face_f[i] = RefitQuad{unit ? rx / l : rx, unit ? ry / l : ry, unit ? rz / l : rz, l};
    if (face_r) face_r[i] = RefitQuad{rx, ry, rz, 0.0f};
}

// Corner c of face i = c / 3, in group g = corner_group[c]: the members of g are member_face[group_first[g] .. group_first[g + 1]) -- the
// FACES of the group's corners, in ascending corner order, a face once per corner it has in the group.  The sum runs in that order; a
// member counts when its face's f is within the crease of f_i (a NaN dot product fails the test).  face_r null: the unit weighting
PT_NRM_HD void normals_corner(const uint32_t* corner_group, const uint32_t* group_first, const uint32_t* member_face, const RefitQuad* face_f,
                              const RefitQuad* face_r, float crease_cos, uint32_t c, float* normals) {
    const RefitQuad fi = face_f[c / 3u];
    const uint32_t g = corner_group[c];
    const uint32_t first = group_first[g], end = group_first[g + 1u];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (uint32_t m = first; m < end; ++m) {
        const uint32_t j = member_face[m];
        const RefitQuad fj = face_f[j];
        const float d = (fj.x * fi.x + fj.y * fi.y) + fj.z * fi.z;
        if (d >= crease_cos) {
            const RefitQuad t = face_r ? face_r[j] : fj;
            sx += t.x; sy += t.y; sz += t.z;
        }
    }
    const float L = __builtin_sqrtf((sx * sx + sy * sy) + sz * sz);
    const bool ok = L > 0.0f;
    reinterpret_cast<RefitQuad*>(normals)[c] = RefitQuad{ok ? sx / L : fi.x, ok ? sy / L : fi.y, ok ? sz / L : fi.z, 0.0f};
}

// ---- host only ----------------------------------------------------------------------------------------------------------------------------------

// prt_weld_corners: corners whose positions are bit-identical after x + 0.0f per component (-0 equals +0: the key of smooth_missing_normals)
// form one group; groups are numbered by first appearance in corner order.  false: a non-finite x, y or z (nothing of the outputs is defined)
inline bool normals_weld(const float* vertices, uint32_t n_tris, uint32_t* corner_group, uint32_t* n_groups) {
    struct Key { uint32_t x, y, z; bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; } };
    struct Hash {
        size_t operator()(const Key& k) const {
            uint64_t h = k.x * 0x9E3779B97F4A7C15ull;
            h = (h ^ (h >> 29) ^ k.y) * 0xBF58476D1CE4E5B9ull;
            h = (h ^ (h >> 32) ^ k.z) * 0x94D049BB133111EBull;
            return (size_t)(h ^ (h >> 31));
        }
    };
    const size_t n = 3 * (size_t)n_tris;
    std::unordered_map<Key, uint32_t, Hash> at;
    at.reserve(n / 2 + 1);
    uint32_t next = 0;
    for (size_t c = 0; c < n; ++c) {
        // (plain float reads: a caller's host array need not be 16-byte aligned)
        const float z0 = vertices[4 * c] + 0.0f, z1 = vertices[4 * c + 1] + 0.0f, z2 = vertices[4 * c + 2] + 0.0f;
        const float fmax = 3.4028234663852886e+38f;
        if (!(__builtin_fabsf(z0) <= fmax && __builtin_fabsf(z1) <= fmax && __builtin_fabsf(z2) <= fmax)) return false;
        Key k;
        std::memcpy(&k.x, &z0, 4); std::memcpy(&k.y, &z1, 4); std::memcpy(&k.z, &z2, 4);
        const auto it = at.emplace(k, next);
        if (it.second) ++next;
        corner_group[c] = it.first->second;
    }
    *n_groups = next;
    return true;
}

// the group-to-members table of prt_set_smooth_normals, by a stable counting sort: group_first [n_groups + 1], member_face [3T] = the face
// (corner / 3) of every corner, the corners of one group together and in ascending corner order; an id no corner names has an empty span.
// false: an id >= n_groups (the outputs are then unspecified)
inline bool normals_group_table(const uint32_t* corner_group, uint32_t n_tris, uint32_t n_groups, std::vector<uint32_t>& group_first,
                                std::vector<uint32_t>& member_face) {
    const size_t n = 3 * (size_t)n_tris;
    group_first.assign((size_t)n_groups + 1u, 0u);
    for (size_t c = 0; c < n; ++c) {
        if (corner_group[c] >= n_groups) return false;
        ++group_first[(size_t)corner_group[c] + 1u];
    }
    for (size_t g = 0; g < n_groups; ++g) group_first[g + 1] += group_first[g];
    std::vector<uint32_t> at(group_first.begin(), group_first.end() - 1);
    member_face.assign(n, 0u);
    for (size_t c = 0; c < n; ++c) member_face[at[corner_group[c]]++] = (uint32_t)(c / 3u);
    return true;
}

}  // namespace prt
