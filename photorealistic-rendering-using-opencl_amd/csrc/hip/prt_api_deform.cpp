// prt_api_deform.cpp -- the calls of the C ABI (include/prt.h) that PRODUCE vertices or normals on the device for the two entry paths of
// prt_api_scene.cpp (update + refit, rebuild): the smoothing topology, the skin and its poses, the morph targets and their morphs, alone or
// in front of the skin.  A deformer writes buffers of its own and enters a path through the path's public device door, as a caller would.
#include <cmath>
#include <new>

#include "prt_ctx.h"
#include "pt_morph.h"
#include "pt_normals.h"
#include "pt_pose.h"

// a new set into fresh buffers: the first hipError_t of a sequence of allocations and uploads (what follows a failure is skipped), sizes in
// records of the buffer's type.  The caller fills a local set and move-assigns it once done() has returned PRT_OK: everything the feature
// will ever need is there, and a failure leaves the set in force as it was
struct Fresh {
    hipError_t e = hipSuccess;
    template <typename T> Fresh& alloc(DevBuf<T>& b, size_t n, bool wanted = true) { if (e == hipSuccess && wanted) e = b.alloc(n); return *this; }
    template <typename T> Fresh& upload(DevBuf<T>& b, const T* src, size_t n, bool wanted = true) { if (e == hipSuccess && wanted) e = b.upload(src, n); return *this; }
    int done(prt_ctx* c, const char* who) {
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) c->err = std::string(who) + ": " + hipGetErrorString(e);
        return e == hipSuccess ? PRT_OK : PRT_ERR_HIP;
    }
};

// a set turned off: nothing of the scene changes, the buffers go
template <typename Set>
static int turn_off(prt_ctx* c, Set& set) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    set = Set{};
    return PRT_OK;
}

// the refusals of the six deformer doors that come before the path they enter: what is not ready first, then the arguments.  A door needs
// the skin and takes matrices, needs the set and takes weights, or both (the fused doors; they have always tested the mode in front of the
// matrices, a pose alone behind them)
enum : unsigned { SKIN = 1u, SET = 2u, FUSED = SKIN | SET };
static int door_checks(prt_ctx* c, const char* who, unsigned needs, const void* matrices, const void* weights, uint32_t mode) {
    const std::string w(who);
    const Scene& sn = c->scene;
    if ((needs & SET) && (!c->have_scene || !sn.morph.on)) return fail(c, PRT_ERR_NOT_READY, w + ": no morph targets set (prt_set_morph_targets)");
    if ((needs & SKIN) && (!c->have_scene || !sn.skin.on)) return fail(c, PRT_ERR_NOT_READY, w + ": no skin set (prt_set_skin)");
    if ((needs & SET) && !weights) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": null weights");
    if (needs == SKIN && !matrices) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": null matrices");
    if (mode != PRT_POSE_REFIT && mode != PRT_POSE_REBUILD) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": unknown mode (the scene is unchanged)");
    if (needs != FUSED) return PRT_OK;
    if (!matrices) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": null matrices");
    if (!sn.skin.rest_n != !sn.morph.base_n) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": exactly one of the skin and the morph set has normals");
    return PRT_OK;
}

// the deformed arrays, in buffers of the context, enter the path `mode` names as a caller's would: the finite-vertex check, the snapshot, the
// guides, the tile orders, the generated normals and the rebuild policy are the path's.  Smooth normals on, or none in the set: it is given none
static int enter_path(prt_ctx* c, const float* v, const float* n, bool has_normals, uint32_t mode, uint32_t max_leaf) {
    if (c->scene.smooth.on || !has_normals) n = nullptr;
    const int rc = mode == PRT_POSE_REFIT ? prt_update_vertices_device(c, v, n) : prt_rebuild_bvh_device(c, v, n, max_leaf);
    if (rc) (void)hipStreamSynchronize(c->stream);         // (a path that refuses before its own wait: the caller's matrices and weights may be reused on return)
    return rc;
}

// what the last pose or morph, accepted or refused, wrote (float4[3T] each; out_n null: the set has no normals)
static int read_deformed(prt_ctx* c, const char* who, bool written, const char* not_yet, const char* no_normals, const float* out_v, const float* out_n,
                  float* vertices, float* normals) {
    const std::string w(who);
    if (!written) return fail(c, PRT_ERR_NOT_READY, w + not_yet);
    if (!vertices) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": null vertices");
    if (normals && !out_n) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + no_normals);
    if (int rc = prt_synchronize(c)) return rc;
    const size_t bytes = 3 * (size_t)c->scene.n_tris * 4 * sizeof(float);
    HIPCHK(c, hipMemcpy(vertices, out_v, bytes, hipMemcpyDeviceToHost));
    if (normals) HIPCHK(c, hipMemcpy(normals, out_n, bytes, hipMemcpyDeviceToHost));
    return PRT_OK;
}

static MorphTables morph_tables(const prt_ctx* c) {
    const MorphSet& ms = c->scene.morph;
    MorphTables t;
    t.base_v = ms.base_v; t.base_n = ms.base_n; t.offset = ms.offset; t.entry_p = ms.entry_p; t.entry_n = ms.entry_n; t.n_tris = c->scene.n_tris;
    t.planes = ms.layout == PRT_MORPH_LAYOUT_PLANES;
    t.block_first = ms.block_first; t.plane_head = ms.plane_head.get(); t.plane_p = ms.plane_p; t.plane_n = ms.plane_n;
    return t;
}

// ---- smooth shading normals regenerated from new vertices (prt.h prt_set_smooth_normals; pt_normals.hip; generated by the entry paths) ---------
extern "C" int prt_set_smooth_normals(prt_ctx* c, const uint32_t* corner_group, uint32_t n_groups, uint32_t weighting, float crease_cos) {
    CTX_CHECK(c);
    if (!c->have_scene || c->scene.n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_set_smooth_normals: no scene with triangles uploaded");
    HIPCHK(c, hipSetDevice(c->device));
    if (!corner_group) return turn_off(c, c->scene.smooth);
    // every refusal before anything of the topology in force is touched
    if (n_groups == 0) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_smooth_normals: n_groups is 0 (the topology in force stays)");
    if (weighting != PRT_NORMALS_UNIT && weighting != PRT_NORMALS_AREA)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_smooth_normals: unknown weighting (the topology in force stays)");
    if (!std::isfinite(crease_cos)) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_smooth_normals: crease_cos is not finite (the topology in force stays)");
    const uint32_t T = c->scene.n_tris;
    if (T > PRT_MAX_TRIANGLE_SLOTS)
        return fail(c, PRT_ERR_UNSUPPORTED, "prt_set_smooth_normals: more than PRT_MAX_TRIANGLE_SLOTS triangles (corners are addressed by 32-bit indices)");
    std::vector<uint32_t> group_first, member_face;
    bool ids_ok = false;
    try { ids_ok = normals_group_table(corner_group, T, n_groups, group_first, member_face); }
    catch (const std::bad_alloc&) { return fail(c, PRT_ERR_UNSUPPORTED, "prt_set_smooth_normals: no host memory for a table of n_groups + 1 entries (the topology in force stays)"); }
    if (!ids_ok) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_smooth_normals: a group id >= n_groups (the topology in force stays)");
    const size_t corners = 3 * (size_t)T;
    Smooth sm;
    Fresh f;
    f.upload(sm.group, corner_group, corners)
     .upload(sm.first, group_first.data(), group_first.size())
     .upload(sm.member, member_face.data(), member_face.size())
     .alloc(sm.face_f, T)
     .alloc(sm.face_r, T, weighting == PRT_NORMALS_AREA)
     .alloc(sm.nrm, 4 * corners);
    if (int rc = f.done(c, "prt_set_smooth_normals")) return rc;
    sm.weighting = weighting; sm.crease = crease_cos;
    sm.on = true;
    c->scene.smooth = std::move(sm);
    return PRT_OK;
}

// ---- the mesh posed on the device from the frame's bone matrices (prt.h prt_set_skin / prt_pose; pt_pose.hip) ----------------------------------
extern "C" int prt_set_skin(prt_ctx* c, const prt_skin* skin) {
    CTX_CHECK(c);
    if (!c->have_scene || c->scene.n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_set_skin: no scene with triangles uploaded");
    HIPCHK(c, hipSetDevice(c->device));
    if (!skin) return turn_off(c, c->scene.skin);
    // every refusal before anything of the skin in force is touched
    const uint32_t T = c->scene.n_tris;
    if (T > PRT_MAX_TRIANGLE_SLOTS)
        return fail(c, PRT_ERR_UNSUPPORTED, "prt_set_skin: more than PRT_MAX_TRIANGLE_SLOTS triangles (corners are addressed by 32-bit indices)");
    if (const char* m = pose_skin_error(skin->rest_vertices, skin->rest_normals, skin->bone_index, skin->bone_weight, skin->n_bones, T))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, std::string("prt_set_skin: ") + m + " (the skin in force stays)");
    const size_t lanes = 4 * 3 * (size_t)T;                // four per corner: of a float4, of the indices, of the weights
    const bool nrm = skin->rest_normals != nullptr;
    Skin sk;
    Fresh f;
    f.upload(sk.rest_v, skin->rest_vertices, lanes)
     .upload(sk.rest_n, skin->rest_normals, lanes, nrm)
     .upload(sk.index, skin->bone_index, lanes)
     .upload(sk.weight, skin->bone_weight, lanes)
     .alloc(sk.mats, 12 * (size_t)skin->n_bones)
     .alloc(sk.out_v, lanes)
     .alloc(sk.out_n, lanes, nrm);
    if (int rc = f.done(c, "prt_set_skin")) return rc;
    sk.n_bones = skin->n_bones;
    sk.on = true;
    c->scene.skin = std::move(sk);
    return PRT_OK;
}

extern "C" int prt_pose_device(prt_ctx* c, const void* d_matrices, uint32_t mode, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = door_checks(c, "prt_pose_device", SKIN, d_matrices, nullptr, mode)) return rc;
    if (!aligned16(d_matrices)) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_pose_device: the matrices must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    Skin& sk = c->scene.skin;
    // the posed arrays into the skin's own buffers: only scratch of the context is written
    PoseTables t;
    t.rest_v = sk.rest_v; t.rest_n = sk.rest_n; t.bone_index = sk.index; t.bone_weight = sk.weight; t.n_tris = c->scene.n_tris;
    launch_pose(t, static_cast<const float*>(d_matrices), sk.out_v, sk.out_n, c->stream);
    HIPCHK(c, hipGetLastError());
    sk.posed = true;
    return enter_path(c, sk.out_v, sk.out_n, sk.rest_n != nullptr, mode, max_leaf);
}

extern "C" int prt_pose(prt_ctx* c, const float* matrices, uint32_t mode, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = door_checks(c, "prt_pose", SKIN, matrices, nullptr, mode)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->scene.skin.mats, matrices, 12 * (size_t)c->scene.skin.n_bones * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return prt_pose_device(c, c->scene.skin.mats, mode, max_leaf);
}

extern "C" int prt_read_posed(prt_ctx* c, float* vertices, float* normals) {
    CTX_CHECK(c);
    const Skin& sk = c->scene.skin;
    return read_deformed(c, "prt_read_posed", c->have_scene && sk.on && sk.posed, ": no pose yet (prt_set_skin, prt_pose)",
                         ": the skin has no rest normals: normals must be NULL", sk.out_v, sk.rest_n ? sk.out_n.get() : nullptr, vertices, normals);
}

// ---- the mesh morphed on the device from the frame's target weights, alone or in front of the skin (prt.h prt_set_morph_targets; pt_morph.hip) --
extern "C" int prt_set_morph_targets_layout(prt_ctx* c, const prt_morph_set* set, uint32_t layout) {
    CTX_CHECK(c);
    if (!c->have_scene || c->scene.n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_set_morph_targets: no scene with triangles uploaded");
    if (layout != PRT_MORPH_LAYOUT_CORNERS && layout != PRT_MORPH_LAYOUT_PLANES)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_morph_targets_layout: unknown layout (the set in force stays)");
    HIPCHK(c, hipSetDevice(c->device));
    if (!set) return turn_off(c, c->scene.morph);
    // every refusal before anything of the set in force is touched
    const uint32_t T = c->scene.n_tris;
    int code = PRT_OK;
    if (const char* m = morph_set_error(set, T, &code)) return fail(c, code, std::string("prt_set_morph_targets: ") + m + " (the set in force stays)");
    const bool planes = layout == PRT_MORPH_LAYOUT_PLANES;
    MorphTable tab;
    MorphPlanes pl;
    try {
        if (planes) morph_build_planes(set, T, pl); else morph_build_table(set, T, tab);
    } catch (const std::bad_alloc&) {
        return fail(c, PRT_ERR_UNSUPPORTED, planes ? "prt_set_morph_targets: out of host memory for the plane table (the set in force stays)"
                                                   : "prt_set_morph_targets: out of host memory for the per-corner table (the set in force stays)");
    }
    const size_t lanes = 4 * 3 * (size_t)T;                // of a float4 per corner
    const bool nrm = set->base_normals != nullptr;
    MorphSet ms;
    Fresh f;
    f.upload(ms.base_v, set->base_vertices, lanes)
     .upload(ms.base_n, set->base_normals, lanes, nrm)
     .upload(ms.offset, tab.offset.data(), tab.offset.size(), !planes)
     .upload(ms.entry_p, reinterpret_cast<const float*>(tab.entry_p.data()), 4 * tab.entry_p.size(), !planes)
     .upload(ms.entry_n, reinterpret_cast<const float*>(tab.entry_n.data()), 4 * tab.entry_n.size(), nrm && !planes)
     .upload(ms.block_first, pl.block_first.data(), pl.block_first.size(), planes)
     .upload(ms.plane_head, reinterpret_cast<const uint4*>(pl.head.data()), pl.head.size(), planes)
     .upload(ms.plane_p, pl.plane_p.data(), pl.plane_p.size(), planes)
     .upload(ms.plane_n, pl.plane_n.data(), pl.plane_n.size(), nrm && planes)
     .alloc(ms.weights, set->n_targets)
     .alloc(ms.out_v, lanes)
     .alloc(ms.out_n, lanes, nrm);
    if (int rc = f.done(c, "prt_set_morph_targets")) return rc;
    ms.layout = layout;
    ms.entries = planes ? pl.entries : (uint64_t)tab.entry_p.size();
    ms.planes = pl.head.size();
    ms.n_targets = set->n_targets;
    ms.on = true;
    c->scene.morph = std::move(ms);
    return PRT_OK;
}

extern "C" int prt_set_morph_targets(prt_ctx* c, const prt_morph_set* set) { return prt_set_morph_targets_layout(c, set, PRT_MORPH_LAYOUT_CORNERS); }

extern "C" int prt_get_morph_report(prt_ctx* c, prt_morph_report* out) {
    CTX_CHECK(c);
    const MorphSet& ms = c->scene.morph;
    if (!c->have_scene || !ms.on) return fail(c, PRT_ERR_NOT_READY, "prt_get_morph_report: no morph targets set (prt_set_morph_targets)");
    if (!out) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_get_morph_report: null out");
    out->layout = ms.layout; out->n_targets = ms.n_targets; out->entries = ms.entries; out->planes = ms.planes;
    out->table_bytes = morph_table_bytes(ms.layout, c->scene.n_tris, ms.entries, ms.planes, ms.base_n != nullptr);
    return PRT_OK;
}

extern "C" int prt_morph_device(prt_ctx* c, const void* d_weights, uint32_t mode, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = door_checks(c, "prt_morph_device", SET, nullptr, d_weights, mode)) return rc;
    if (!aligned16(d_weights)) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_morph_device: the weights must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    MorphSet& ms = c->scene.morph;
    // the morphed arrays into the set's own buffers
    launch_morph(morph_tables(c), static_cast<const float*>(d_weights), ms.out_v, ms.out_n, c->stream);
    HIPCHK(c, hipGetLastError());
    ms.morphed = true;
    return enter_path(c, ms.out_v, ms.out_n, ms.base_n != nullptr, mode, max_leaf);
}

extern "C" int prt_morph(prt_ctx* c, const float* weights, uint32_t mode, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = door_checks(c, "prt_morph", SET, nullptr, weights, mode)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->scene.morph.weights, weights, (size_t)c->scene.morph.n_targets * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return prt_morph_device(c, c->scene.morph.weights, mode, max_leaf);
}

extern "C" int prt_pose_morphed_device(prt_ctx* c, const void* d_matrices, const void* d_weights, uint32_t mode, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = door_checks(c, "prt_pose_morphed_device", FUSED, d_matrices, d_weights, mode)) return rc;
    if (!aligned16(d_matrices) || !aligned16(d_weights))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_pose_morphed_device: the matrices and the weights must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    Skin& sk = c->scene.skin;
    // into the skin's posed buffers, as a pose: prt_read_posed returns them.  The rest pose arrives in registers: the skin's is not read
    PoseTables t;
    t.rest_v = nullptr; t.rest_n = nullptr; t.bone_index = sk.index; t.bone_weight = sk.weight; t.n_tris = c->scene.n_tris;
    launch_pose_morphed(morph_tables(c), t, static_cast<const float*>(d_matrices), static_cast<const float*>(d_weights), sk.out_v, sk.out_n, c->stream);
    HIPCHK(c, hipGetLastError());
    sk.posed = true;
    return enter_path(c, sk.out_v, sk.out_n, sk.rest_n != nullptr, mode, max_leaf);
}

extern "C" int prt_pose_morphed(prt_ctx* c, const float* matrices, const float* weights, uint32_t mode, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = door_checks(c, "prt_pose_morphed", FUSED, matrices, weights, mode)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->scene.skin.mats, matrices, 12 * (size_t)c->scene.skin.n_bones * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->scene.morph.weights, weights, (size_t)c->scene.morph.n_targets * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return prt_pose_morphed_device(c, c->scene.skin.mats, c->scene.morph.weights, mode, max_leaf);
}

extern "C" int prt_read_morphed(prt_ctx* c, float* vertices, float* normals) {
    CTX_CHECK(c);
    const MorphSet& ms = c->scene.morph;
    return read_deformed(c, "prt_read_morphed", c->have_scene && ms.on && ms.morphed, ": no morph yet (prt_set_morph_targets, prt_morph)",
                         ": the set has no base normals: normals must be NULL", ms.out_v, ms.base_n ? ms.out_n.get() : nullptr, vertices, normals);
}
