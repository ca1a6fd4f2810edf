// pt_morph.h -- the body of the morph kernels (pt_morph.hip; prt.h prt_set_morph_targets / prt_morph / prt_pose_morphed): base mesh + sparse
// per-corner deltas of the targets + the frame's weights -> morphed vertices and normals, written as the formulas of prt.h.  Plain pointers
// and __host__ __device__ inline functions only, as pt_pose.h, so that a host harness (tests/emu/morph_emu.cpp) runs the same code serially.
// f32 operations in the order of prt.h, no contraction (build.py: -ffp-contract=off); sqrtf and / are the correctly rounded ones on both sides.
// The host-only part below the body: the checks of prt_set_morph_targets and the builders of the per-corner table and of the plane table.
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

// ---- the plane table (prt.h PRT_MORPH_LAYOUT_PLANES) ---------------------------------------------------------------------------------------------
// Block b is corners 64 b .. 64 b + 63; a plane exists for every (block b, target t) where t lists a corner of b, ordered by (b, t):
// block_first[b] .. block_first[b + 1] are the planes of block b, in ascending t.  A plane is a head and three rows of 64 floats (with
// normals three more): plane_p[192 u + 64 k + l] is component k of dp of lane l of plane u, +0 on a lane the mask does not list.  On the
// device b is wave-uniform (one wave per block), so block_first, the head and the weight are scalar loads, the zero-weight test is a scalar
// branch in front of the plane's rows, and a row is one 256-byte line of 64 lanes
struct alignas(16) MorphPlaneHead { uint32_t target, zero, mask_lo, mask_hi; };
typedef uint32_t MorphHeadWords __attribute__((ext_vector_type(4)));       // a head as it is loaded: x the target, z and w the mask
constexpr uint32_t PT_MORPH_PLANE_FLOATS = 192u;
// The loop takes the planes of a block PT_MORPH_TRIP at a time: the heads of a trip are asked for together, then their weights, then every
// row of those with a non-zero weight, and only then is the first row used -- three waits for memory per trip, not per plane
constexpr uint32_t PT_MORPH_TRIP = 4u;
// the rows of one plane have been loaded into registers at this point of the program, whatever uses them later (the device only: the host
// has no such choice to make).  Left to itself the compiler moves a row's load under the lane's mask bit and waits for it there
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_MORPH_LOADED(d) asm volatile("" : "+v"((d)[0]), "+v"((d)[1]), "+v"((d)[2]), "+v"((d)[3]), "+v"((d)[4]), "+v"((d)[5]))
#else
#define PT_MORPH_LOADED(d) ((void)(d))
#endif

// Lane l of block b: the loop of morph_raw over the planes of the block.  For a listed lane the operands and the order of the additions are
// morph_raw's; for an unlisted one nothing is added (w * +0 would turn a -0 into +0 and a NaN weight into a NaN on every lane of the plane)
PT_MORPH_HD void morph_raw_planes(const uint32_t* block_first, const MorphPlaneHead* plane_head, const float* plane_p, const float* plane_n,
                                  const float* weights, uint32_t b, uint32_t l, RefitQuad& p, RefitQuad& n) {
    const uint32_t first = block_first[b], end = block_first[b + 1];
    for (uint32_t u0 = first; u0 < end; u0 += PT_MORPH_TRIP) {
        // (a plane past the block's last one: the last one again, under a weight of zero)
        // (a head is one 16-byte load: its mask is there before the rows are, not asked for after them)
        MorphHeadWords h[PT_MORPH_TRIP];
        float w[PT_MORPH_TRIP];
#pragma unroll
        for (uint32_t j = 0; j < PT_MORPH_TRIP; ++j) h[j] = reinterpret_cast<const MorphHeadWords*>(plane_head)[u0 + j < end ? u0 + j : end - 1u];
#pragma unroll
        for (uint32_t j = 0; j < PT_MORPH_TRIP; ++j) w[j] = weights[h[j].x];
        uint32_t active = 0;
#pragma unroll
        for (uint32_t j = 0; j < PT_MORPH_TRIP; ++j) {
            if (u0 + j >= end) w[j] = 0.0f;
            active |= w[j] == 0.0f ? 0u : 1u;               // (either sign; a NaN is not zero)
        }
        if (!active) continue;
        float d[PT_MORPH_TRIP][6];
#pragma unroll
        for (uint32_t j = 0; j < PT_MORPH_TRIP; ++j) {
            for (int k = 0; k < 6; ++k) d[j][k] = 0.0f;
            if (w[j] == 0.0f) continue;
            const size_t row = (size_t)(u0 + j) * PT_MORPH_PLANE_FLOATS + l;         // 64-bit: 768 P bytes pass 4 GiB
            d[j][0] = plane_p[row]; d[j][1] = plane_p[row + 64]; d[j][2] = plane_p[row + 128];
            if (plane_n) { d[j][3] = plane_n[row]; d[j][4] = plane_n[row + 64]; d[j][5] = plane_n[row + 128]; }
        }
#pragma unroll
        for (uint32_t j = 0; j < PT_MORPH_TRIP; ++j) PT_MORPH_LOADED(d[j]);
#pragma unroll
        for (uint32_t j = 0; j < PT_MORPH_TRIP; ++j) {
            if (w[j] == 0.0f) continue;
            const uint64_t mask = (uint64_t)h[j].w << 32 | h[j].z;
            const bool on = (mask >> l) & 1u;
            const float wj = w[j];
            p.x = on ? p.x + wj * d[j][0] : p.x; p.y = on ? p.y + wj * d[j][1] : p.y; p.z = on ? p.z + wj * d[j][2] : p.z;
            if (plane_n) { n.x = on ? n.x + wj * d[j][3] : n.x; n.y = on ? n.y + wj * d[j][4] : n.y; n.z = on ? n.z + wj * d[j][5] : n.z; }
        }
    }
}

// prt_morph and prt_pose_morphed over the plane table: morph_corner's and pose_morphed_corner's loads and tails around the loop above
PT_MORPH_HD void morph_planes_corner(const float* base_v, const float* base_n, const uint32_t* block_first, const MorphPlaneHead* plane_head,
                                     const float* plane_p, const float* plane_n, const float* weights, uint32_t b, uint32_t l, float* out_v,
                                     float* out_n) {
    const size_t c = (size_t)b * 64 + l;
    RefitQuad p = reinterpret_cast<const RefitQuad*>(base_v)[c];
    RefitQuad n{0.0f, 0.0f, 0.0f, 0.0f};
    if (base_n) n = reinterpret_cast<const RefitQuad*>(base_n)[c];
    morph_raw_planes(block_first, plane_head, plane_p, base_n ? plane_n : nullptr, weights, b, l, p, n);
    reinterpret_cast<RefitQuad*>(out_v)[c] = RefitQuad{p.x, p.y, p.z, 0.0f};
    if (base_n) {
        const float L = __builtin_sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
        const bool unit = L > 0.0f;
        reinterpret_cast<RefitQuad*>(out_n)[c] = RefitQuad{unit ? n.x / L : n.x, unit ? n.y / L : n.y, unit ? n.z / L : n.z, 0.0f};
    }
}

PT_MORPH_HD void pose_morphed_planes_corner(const float* base_v, const float* base_n, const uint32_t* block_first, const MorphPlaneHead* plane_head,
                                            const float* plane_p, const float* plane_n, const float* weights, const uint16_t* bone_index,
                                            const float* bone_weight, const float* matrices, uint32_t b, uint32_t l, float* out_v, float* out_n) {
    const size_t c = (size_t)b * 64 + l;
    RefitQuad p = reinterpret_cast<const RefitQuad*>(base_v)[c];
    RefitQuad n{0.0f, 0.0f, 0.0f, 0.0f};
    if (base_n) n = reinterpret_cast<const RefitQuad*>(base_n)[c];
    morph_raw_planes(block_first, plane_head, plane_p, base_n ? plane_n : nullptr, weights, b, l, p, n);
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

// the plane table of an accepted set: the planes of a block in ascending t (the targets are walked in ascending t, a target's corners in
// ascending order).  plane_n stays empty without base normals; a target with d_normal == NULL contributes +0 deltas.  entries: the sum of
// n_entries
struct MorphPlanes {
    std::vector<uint32_t> block_first;        // ceil(3T / 64) + 1
    std::vector<MorphPlaneHead> head;
    std::vector<float> plane_p, plane_n;      // 192 per plane
    uint64_t entries = 0;
};

inline uint64_t morph_entries(const prt_morph_set* set) {
    uint64_t total = 0;
    for (uint32_t t = 0; t < set->n_targets; ++t) total += set->targets[t].n_entries;
    return total;
}

inline void morph_build_planes(const prt_morph_set* set, uint32_t n_tris, MorphPlanes& out) {
    const size_t n = 3 * (size_t)n_tris, blocks = (n + 63) / 64;
    const uint32_t none = 0xFFFFFFFFu;
    out.entries = morph_entries(set);
    out.block_first.assign(blocks + 1, 0u);
    for (uint32_t t = 0; t < set->n_targets; ++t) {
        const prt_morph_target& g = set->targets[t];
        uint32_t last = none;
        for (uint32_t j = 0; j < g.n_entries; ++j) {
            const uint32_t b = g.corner[j] >> 6;
            if (b != last) { ++out.block_first[(size_t)b + 1]; last = b; }
        }
    }
    for (size_t b = 0; b < blocks; ++b) out.block_first[b + 1] += out.block_first[b];
    const size_t planes = out.block_first[blocks];
    const bool nrm = set->base_normals != nullptr;
    out.head.assign(planes, MorphPlaneHead{0u, 0u, 0u, 0u});
    out.plane_p.assign(planes * PT_MORPH_PLANE_FLOATS, 0.0f);
    out.plane_n.assign(nrm ? planes * PT_MORPH_PLANE_FLOATS : 0, 0.0f);
    std::vector<uint32_t> cursor(out.block_first.begin(), out.block_first.end() - 1);
    for (uint32_t t = 0; t < set->n_targets; ++t) {
        const prt_morph_target& g = set->targets[t];
        uint32_t last = none;
        size_t u = 0;
        for (size_t j = 0; j < g.n_entries; ++j) {
            const uint32_t b = g.corner[j] >> 6, l = g.corner[j] & 63u;
            if (b != last) { u = cursor[b]++; out.head[u].target = t; last = b; }
            if (l < 32u) out.head[u].mask_lo |= 1u << l; else out.head[u].mask_hi |= 1u << (l - 32u);
            float* row = out.plane_p.data() + u * PT_MORPH_PLANE_FLOATS + l;
            row[0] = g.d_position[4 * j]; row[64] = g.d_position[4 * j + 1]; row[128] = g.d_position[4 * j + 2];
            if (nrm && g.d_normal) {
                row = out.plane_n.data() + u * PT_MORPH_PLANE_FLOATS + l;
                row[0] = g.d_normal[4 * j]; row[64] = g.d_normal[4 * j + 1]; row[128] = g.d_normal[4 * j + 2];
            }
        }
    }
}

// prt_get_morph_report's table_bytes (prt.h): the device bytes of the delta tables alone
inline uint64_t morph_table_bytes(uint32_t layout, uint32_t n_tris, uint64_t entries, uint64_t planes, bool nrm) {
    const uint64_t n = 3 * (uint64_t)n_tris, k = nrm ? 2u : 1u;
    return layout == PRT_MORPH_LAYOUT_PLANES ? 4 * ((n + 63) / 64 + 1) + 16 * planes + 768 * planes * k : 4 * (n + 1) + 16 * entries * k;
}

}  // namespace prt
