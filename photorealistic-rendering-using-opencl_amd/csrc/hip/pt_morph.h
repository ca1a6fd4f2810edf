// pt_morph.h -- the body of the morph kernels (pt_morph.hip; prt.h prt_set_morph_targets / prt_morph / prt_pose_morphed): base mesh + sparse
// per-corner deltas of the targets + the frame's weights -> morphed vertices and normals, written as the formulas of prt.h.  Plain pointers
// and __host__ __device__ inline functions only, as pt_pose.h, so that a host harness (tests/emu/morph_emu.cpp) runs the same code serially.
// f32 operations in the order of prt.h, no contraction (build.py: -ffp-contract=off); sqrtf and / are the correctly rounded ones on both sides.
// The host-only part below the body: the checks of prt_set_morph_targets and the builder of the per-corner table.
#pragma once
#include <stdint.h>

#include "pt_pose.h"              // pose_values: the fused kernel poses the morphed rest pose in registers

#define PT_MORPH_HD PT_REFIT_HD

namespace prt {

constexpr uint32_t PT_MORPH_MAX_TARGETS = 65536u;

// The table is a CSR over corners: the entries of corner c are records offset[c] .. offset[c + 1], sorted by target.  A record is 16 bytes,
// {dp.x, dp.y, dp.z, the target's number as the bits of lane 3}: one 16-byte load; with normals a parallel float4 array holds dn.
// Consecutive lanes own consecutive corners, and consecutive corners own consecutive records.  The weight table (4 bytes per target, at
// most 256 KiB) stays in global memory and is read through the vector cache at a per-lane index, as the matrix table of pt_pose.h is.
PT_MORPH_HD uint32_t morph_target_of(const RefitQuad& rec) {
    uint32_t t;
    __builtin_memcpy(&t, &rec.w, 4);
    return t;
}

// Corner c: p = base position, n = base normal (entry_n null: n is left alone); for each of its entries in ascending target order with
// w = weights[t] != 0 (a zero of either sign skips the entry): p.i = p.i + w * dp.i, n.i = n.i + w * dn.i.  Lane 3 of p and n is whatever
// the base holds: the callers write 0
PT_MORPH_HD void morph_raw(const uint32_t* offset, const float* entry_p, const float* entry_n, const float* weights, size_t c, RefitQuad& p,
                           RefitQuad& n) {
    const uint32_t first = offset[c], end = offset[c + 1];
    for (uint32_t e = first; e < end; ++e) {
        const RefitQuad d = reinterpret_cast<const RefitQuad*>(entry_p)[e];
        const float w = weights[morph_target_of(d)];
        // (selects, not a branch around the position: the record, which holds the target's number, stays one 16-byte load.  The normal
        // delta is only loaded under a weight)
        const bool on = w != 0.0f;
        p.x = on ? p.x + w * d.x : p.x; p.y = on ? p.y + w * d.y : p.y; p.z = on ? p.z + w * d.z : p.z;
        if (on && entry_n) {
            const RefitQuad dn = reinterpret_cast<const RefitQuad*>(entry_n)[e];
            n.x = n.x + w * dn.x; n.y = n.y + w * dn.y; n.z = n.z + w * dn.z;
        }
    }
}

// prt_morph: vertex = {p, 0}; L = |n|, normal = L > 0 ? n / L : n, lane 3 = 0.  base_n null: no normals (entry_n is not read, out_n is not
// written)
PT_MORPH_HD void morph_corner(const float* base_v, const float* base_n, const uint32_t* offset, const float* entry_p, const float* entry_n,
                              const float* weights, size_t c, float* out_v, float* out_n) {
    RefitQuad p = reinterpret_cast<const RefitQuad*>(base_v)[c];
    RefitQuad n{0.0f, 0.0f, 0.0f, 0.0f};
    if (base_n) n = reinterpret_cast<const RefitQuad*>(base_n)[c];
    morph_raw(offset, entry_p, base_n ? entry_n : nullptr, weights, c, p, n);
    reinterpret_cast<RefitQuad*>(out_v)[c] = RefitQuad{p.x, p.y, p.z, 0.0f};
    if (base_n) {
        const float L = __builtin_sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
        const bool unit = L > 0.0f;
        reinterpret_cast<RefitQuad*>(out_n)[c] = RefitQuad{unit ? n.x / L : n.x, unit ? n.y / L : n.y, unit ? n.z / L : n.z, 0.0f};
    }
}

// prt_pose_morphed: the morphed p and n, un-normalised, take the place of the skin's rest pose in pt_pose.h's formulas.  They never go to
// memory
PT_MORPH_HD void pose_morphed_corner(const float* base_v, const float* base_n, const uint32_t* offset, const float* entry_p, const float* entry_n,
                                     const float* weights, const uint16_t* bone_index, const float* bone_weight, const float* matrices, size_t c,
                                     float* out_v, float* out_n) {
    RefitQuad p = reinterpret_cast<const RefitQuad*>(base_v)[c];
    RefitQuad n{0.0f, 0.0f, 0.0f, 0.0f};
    if (base_n) n = reinterpret_cast<const RefitQuad*>(base_n)[c];
    morph_raw(offset, entry_p, base_n ? entry_n : nullptr, weights, c, p, n);
    const RefitQuad wq = reinterpret_cast<const RefitQuad*>(bone_weight)[c];
    const PoseIndex idx = reinterpret_cast<const PoseIndex*>(bone_index)[c];
    pose_values(p, base_n != nullptr, [=]() { return n; }, wq, idx, matrices, c, out_v, out_n);
}

}  // namespace prt

// ---- host only ----------------------------------------------------------------------------------------------------------------------------------
#include <vector>

#include "prt.h"

namespace prt {

// the refusals of prt_set_morph_targets over the caller's host arrays (plain reads: they need not be aligned); null = accepted, else what
// is wrong, with PRT_ERR_INVALID_ARGUMENT or PRT_ERR_UNSUPPORTED in *code.  Everything that bounds a read is checked before the read
inline const char* morph_set_error(const prt_morph_set* set, uint32_t n_tris, int* code) {
    *code = PRT_ERR_INVALID_ARGUMENT;
    if (!set->base_vertices || !set->targets) return "null base_vertices or targets";
    if (set->n_targets < 1u || set->n_targets > PT_MORPH_MAX_TARGETS) return "n_targets outside 1 .. 65536";
    const uint64_t n = 3 * (uint64_t)n_tris;
    uint64_t total = 0;
    for (uint32_t t = 0; t < set->n_targets; ++t) {
        const prt_morph_target& g = set->targets[t];
        if (g.n_entries && (!g.corner || !g.d_position)) return "a target with entries and a null corner or d_position";
        if (g.n_entries > n) return "a target with more entries than the mesh has corners (corners are strictly ascending)";
        total += g.n_entries;
    }
    if (n_tris > PRT_MAX_TRIANGLE_SLOTS) { *code = PRT_ERR_UNSUPPORTED; return "more than PRT_MAX_TRIANGLE_SLOTS triangles (corners are addressed by 32-bit indices)"; }
    if (total > 0xFFFFFFFFull) { *code = PRT_ERR_UNSUPPORTED; return "more than 2^32 - 1 entries in total (the table's offsets are 32-bit)"; }
    const float fmax = 3.4028234663852886e+38f;
    for (uint32_t t = 0; t < set->n_targets; ++t) {
        const prt_morph_target& g = set->targets[t];
        for (uint32_t j = 0; j < g.n_entries; ++j) {
            if (g.corner[j] >= n) return "a corner >= 3T";
            if (j && g.corner[j] <= g.corner[j - 1]) return "corners of a target that are not strictly ascending";
        }
    }
    for (uint64_t c = 0; c < n; ++c)
        for (int k = 0; k < 3; ++k) {
            if (!(__builtin_fabsf(set->base_vertices[4 * c + k]) <= fmax)) return "a base vertex with a non-finite x, y or z";
            if (set->base_normals && !(__builtin_fabsf(set->base_normals[4 * c + k]) <= fmax)) return "a base normal with a non-finite component";
        }
    for (uint32_t t = 0; t < set->n_targets; ++t) {
        const prt_morph_target& g = set->targets[t];
        for (uint64_t j = 0; j < g.n_entries; ++j)
            for (int k = 0; k < 3; ++k) {
                if (!(__builtin_fabsf(g.d_position[4 * j + k]) <= fmax)) return "a position delta that is not finite";
                if (set->base_normals && g.d_normal && !(__builtin_fabsf(g.d_normal[4 * j + k]) <= fmax)) return "a normal delta that is not finite";
            }
    }
    return nullptr;
}

// the device tables of an accepted set (morph_set_error returned null): a stable counting sort of the entries by corner over the targets in
// ascending t, so the entries of a corner are in ascending t.  entry_n stays empty without base normals; a target with d_normal == NULL
// contributes +0 deltas
struct MorphTable {
    std::vector<uint32_t> offset;             // 3T + 1
    std::vector<RefitQuad> entry_p, entry_n;
};

inline void morph_build_table(const prt_morph_set* set, uint32_t n_tris, MorphTable& out) {
    const size_t n = 3 * (size_t)n_tris;
    out.offset.assign(n + 1, 0u);
    for (uint32_t t = 0; t < set->n_targets; ++t) {
        const prt_morph_target& g = set->targets[t];
        for (uint32_t j = 0; j < g.n_entries; ++j) ++out.offset[(size_t)g.corner[j] + 1];
    }
    for (size_t c = 0; c < n; ++c) out.offset[c + 1] += out.offset[c];
    const size_t total = out.offset[n];
    out.entry_p.assign(total, RefitQuad{0.0f, 0.0f, 0.0f, 0.0f});
    out.entry_n.assign(set->base_normals ? total : 0, RefitQuad{0.0f, 0.0f, 0.0f, 0.0f});
    std::vector<uint32_t> cursor(out.offset.begin(), out.offset.end() - 1);
    for (uint32_t t = 0; t < set->n_targets; ++t) {
        const prt_morph_target& g = set->targets[t];
        float id;
        __builtin_memcpy(&id, &t, 4);
        for (size_t j = 0; j < g.n_entries; ++j) {
            const uint32_t e = cursor[g.corner[j]]++;
            out.entry_p[e] = RefitQuad{g.d_position[4 * j], g.d_position[4 * j + 1], g.d_position[4 * j + 2], id};
            if (set->base_normals && g.d_normal) out.entry_n[e] = RefitQuad{g.d_normal[4 * j], g.d_normal[4 * j + 1], g.d_normal[4 * j + 2], 0.0f};
        }
    }
}

}  // namespace prt
