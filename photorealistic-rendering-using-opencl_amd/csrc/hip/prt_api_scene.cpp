// prt_api_scene.cpp -- the scene calls of the C ABI (include/prt.h): upload, the two entry paths of new vertices (update with a refit,
// rebuild) with the normals they generate, the primitives, the tree's cost and rebuild policy, motion on / off and the tree's read-backs.
// What produces vertices or normals for the two paths -- the smoothing topology, the skin, the morph targets -- is in prt_api_deform.cpp.
#include <cmath>
#include <utility>

#include "prt_ctx.h"
#include "pt_build.h"
#include "pt_pack.h"
#include "pt_refit.h"

extern "C" int prt_upload_scene(prt_ctx* c, const prt_scene_desc* s) {
    CTX_CHECK(c);
    // everything that can be refused is refused before the old scene is touched (pt_pack.cpp: pure host code)
    PackedScene ps;
    std::string perr;
    int rc = pack_scene(c->cfg, s, ps, perr);
    if (rc) return fail(c, rc, perr);
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->stream);
    // from here on the old scene is gone: the context has none until every upload has succeeded.  (A static scene holds no refit tables or
    // staging buffers on the device; snapshots and the smoothing topology were the old scene's.  The map, the spare tree set and the build's
    // scratch are the context's and stay)
    c->have_scene = false;
    c->frame.guides_valid = false;
    c->frame.hist.valid = false;
    c->scene = Scene{};
    c->sc = DevScene{};
    bind(c);
    Scene& sn = c->scene;
    sn.mesh_t.resize(s->object_count[7]);
    for (uint32_t i = 0; i < s->object_count[7]; ++i) sn.mesh_t[i] = s->meshes[i].t;
    sn.n_slots = ps.slot_vtx.size();
    if (s->triangle_count) {
        sn.up_nodes.assign(s->bvh_nodes, s->bvh_nodes + s->bvh_node_count);
        sn.up_prims.assign(s->primitive_indices, s->primitive_indices + s->triangle_count);
    }
    sn.slot_vtx.swap(ps.slot_vtx); sn.level_pairs.swap(ps.level_pairs); sn.level_first.swap(ps.level_first); sn.node_box.swap(ps.node_box);
    std::memcpy(sn.root_bounds, ps.root_bounds, sizeof(sn.root_bounds));
    sn.n_tris = s->triangle_count; sn.n_nodes = s->triangle_count ? s->bvh_node_count : 0u;
    HIPCHK(c, sn.tree.pairs.upload(ps.pairs));
    HIPCHK(c, sn.tree.tri_geom.upload(ps.tg));
    HIPCHK(c, sn.tree.tri_nrm.upload(ps.tn));
    HIPCHK(c, sn.spheres.upload(ps.spheres));
    HIPCHK(c, sn.quads.upload(ps.quads));
    HIPCHK(c, sn.sdfs.upload(ps.sdfs));
    HIPCHK(c, sn.mats.upload(ps.mats));
    HIPCHK(c, sn.light_tab.upload(ps.light_tab));
    c->sc = ps.sc;
    bind(c);
    if (!c->ctx.env) {
        const float black[3] = {0.f, 0.f, 0.f};
        rc = prt_upload_envmap(c, black, 1, 1);
        if (rc) return rc;
    }
    c->have_scene = true;
    forget_tile_orders(c);
    return PRT_OK;
}

// ---- deforming geometry: new vertices into the uploaded tree (prt.h prt_update_vertices; pt_refit.hip) ----------------------------------------

// the size limits of the tables a refit or a rebuild writes and the render kernels read by 32-bit offsets (prt.h PRT_MAX_*; pt_layout.h)
static int table_limits(prt_ctx* c, const std::string& who, uint64_t slots, uint64_t pairs) {
    const char* m = table_limit_error(slots, pairs, (uint64_t)c->sc.n_meshes + 2u);
    return m ? fail(c, PRT_ERR_UNSUPPORTED, who + ": " + m) : PRT_OK;
}

// the checks both variants share, and the device tables on the first update
static int refit_prepare(prt_ctx* c, const void* vertices, const char* who) {
    const std::string w(who);
    if (!c->have_scene || c->scene.n_tris == 0) return fail(c, PRT_ERR_NOT_READY, w + ": no scene with triangles uploaded");
    if (!vertices) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": null vertices");
    if (!c->sc.root_is_leaf && c->scene.level_first.size() > 257u)
        return fail(c, PRT_ERR_UNSUPPORTED, w + ": the tree has more than 256 levels of pairs (one launch per level)");
    if (int rc = table_limits(c, w, c->scene.n_slots, c->sc.n_pairs)) return rc;       // (the tables the refit kernels write)
    HIPCHK(c, hipSetDevice(c->device));
    return refit_tables(c);
}

// the tables of the uploaded tree on the device (a rebuilt tree's are there from its build)
int refit_tables(prt_ctx* c) {
    Scene& sn = c->scene;
    if (sn.refit_ready) return PRT_OK;
    HIPCHK(c, sn.tree.slot_vtx.upload(sn.slot_vtx));
    HIPCHK(c, sn.tree.level_pairs.upload(sn.level_pairs));
    HIPCHK(c, sn.tree.root.alloc(8));
    float init[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::memcpy(init, sn.root_bounds, sizeof(sn.root_bounds));      // (an empty leaf root keeps the box it was uploaded with)
    HIPCHK(c, hipMemcpy(sn.tree.root, init, sizeof(init), hipMemcpyHostToDevice));
    sn.refit_ready = true;
    return PRT_OK;
}

// the host variants' vertices (and normals, unless null) into the staging buffers on the context's stream
static int stage_vertices(prt_ctx* c, const float* vertices, const float* normals) {
    Scene& sn = c->scene;
    const size_t floats = 3 * (size_t)sn.n_tris * 4;
    HIPCHK(c, sn.stage_vtx.first_use(floats));
    if (normals) HIPCHK(c, sn.stage_nrm.first_use(floats));
    HIPCHK(c, hipMemcpyAsync(sn.stage_vtx, vertices, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (normals) HIPCHK(c, hipMemcpyAsync(sn.stage_nrm, normals, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return PRT_OK;
}

// smooth normals on and no normals given (prt.h prt_set_smooth_normals): the normals of the new vertices into the context's own buffer, two
// launches on the context's stream; the caller passes the buffer on as if it had been given.  Called once the finite-vertex check has passed:
// only scratch of the context is written
static const float* generate_normals(prt_ctx* c, const float* v) {
    const Smooth& sm = c->scene.smooth;
    SmoothTables t;
    t.corner_group = sm.group; t.group_first = sm.first; t.member_face = sm.member;
    t.face_f = sm.face_f; t.face_r = sm.face_r;       // (face_r: allocated for the area weighting only)
    t.n_tris = c->scene.n_tris; t.crease_cos = sm.crease;
    launch_smooth_normals(t, v, sm.nrm, c->stream);
    return sm.nrm;
}

// ---- the cost of the current tree, and the rule that rebuilds a refitted tree (prt.h prt_bvh_cost / prt_set_rebuild_policy; pt_cost.hip) ------
// the checks are the caller's: a scene with triangles, the device selected.  The launches on the context's stream, the 8 bytes back, complete
// on return.  Only the scratch is written
static int measure_cost(prt_ctx* c, double* cost) {
    Scene& sn = c->scene;
    HIPCHK(c, sn.cost_work.reserve(cost_work_doubles(c->sc.n_pairs)));
    const double* at = sn.cost_work;
    if (c->sc.root_is_leaf)      // (the root's box: the device's after an update, before one as uploaded)
        launch_bvh_cost_leaf_root(sn.refitted ? sn.tree.root.get() : nullptr, sn.root_bounds, c->sc.root_leaf_count, sn.cost_work, c->stream);
    else
        at = launch_bvh_cost(sn.tree.pairs, c->sc.n_pairs, sn.cost_work, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cost, at, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

extern "C" int prt_bvh_cost(prt_ctx* c, double* cost) {
    CTX_CHECK(c);
    if (!c->have_scene || c->scene.n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_bvh_cost: no scene with triangles uploaded");
    if (!cost) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_bvh_cost: null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    double v = 0.0;
    if (int rc = measure_cost(c, &v)) return rc;
    *cost = v;
    return PRT_OK;
}

extern "C" int prt_set_rebuild_policy(prt_ctx* c, const prt_rebuild_policy* policy) {
    CTX_CHECK(c);
    if (!c->have_scene || c->scene.n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_set_rebuild_policy: no scene with triangles uploaded");
    if (!policy) {                                         // off: nothing of the scene changes
        c->scene.policy = RebuildPolicy{};
        return PRT_OK;
    }
    // every refusal before anything of the policy in force is touched
    if (!std::isfinite(policy->limit) || policy->limit < 1.0f)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_rebuild_policy: limit is not finite or below 1 (the policy in force stays)");
    if (policy->max_leaf > 64u) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_rebuild_policy: max_leaf above 64 (the policy in force stays)");
    if (c->scene.n_tris - 1u > PRT_MAX_NODE_PAIRS)
        return fail(c, PRT_ERR_UNSUPPORTED, "prt_set_rebuild_policy: more than PRT_MAX_NODE_PAIRS + 1 triangles: no rebuild would be accepted (the policy in force stays)");
    HIPCHK(c, hipSetDevice(c->device));
    RebuildPolicy p;
    if (int rc = measure_cost(c, &p.baseline)) return rc;
    p.on = true; p.limit = policy->limit; p.max_leaf = policy->max_leaf;
    p.rep.cost = p.baseline;
    c->scene.policy = p;
    return PRT_OK;
}

extern "C" int prt_get_rebuild_report(prt_ctx* c, prt_rebuild_report* out) {
    CTX_CHECK(c);
    if (!c->have_scene || !c->scene.policy.on) return fail(c, PRT_ERR_NOT_READY, "prt_get_rebuild_report: no rebuild policy set (prt_set_rebuild_policy)");
    if (!out) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_get_rebuild_report: null pointer");
    *out = c->scene.policy.rep;
    out->baseline = c->scene.policy.baseline;              // (in force now: an explicit rebuild since the last refit-path call has moved it)
    return PRT_OK;
}

// the policy's part of an accepted refit: the refitted tree is costed and, past the limit, rebuilt from the same buffers -- the sequence
// update, prt_bvh_cost, prt_rebuild_bvh_device, call for call.  A rebuild that is refused or fails returns its status: the scene is the
// refitted one
static int policy_after_refit(prt_ctx* c, const void* d_vertices, const void* d_normals) {
    RebuildPolicy& p = c->scene.policy;
    double cost = 0.0;
    if (int rc = measure_cost(c, &cost)) return rc;
    p.rep.cost = cost; p.rep.rebuilt = 0;
    if (!(cost > (double)p.limit * p.baseline)) return PRT_OK;       // (a NaN on either side: no rebuild)
    if (int rc = prt_rebuild_bvh_device(c, d_vertices, d_normals, p.max_leaf)) return rc;       // (measures the new baseline)
    p.rep.rebuilt = 1; p.rep.rebuilds += 1;
    return PRT_OK;
}

extern "C" int prt_update_vertices_device(prt_ctx* c, const void* d_vertices, const void* d_normals) {
    CTX_CHECK(c);
    int rc = refit_prepare(c, d_vertices, "prt_update_vertices_device");
    if (rc) return rc;
    if (!aligned16(d_vertices) || !aligned16(d_normals))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_update_vertices_device: the device buffers must be 16-byte aligned");
    const float* v = static_cast<const float*>(d_vertices);
    const float* n = static_cast<const float*>(d_normals);
    Scene& sn = c->scene;
    TreeSet& tree = sn.tree;
    // the check first: its flag is read before anything of the scene is overwritten
    uint32_t* flag = reinterpret_cast<uint32_t*>(tree.root.get()) + 6;
    uint32_t bad = 0;
    if ((rc = checked(c, flag, &bad, 1, [&] { launch_refit_check(v, 3 * (size_t)sn.n_tris, flag, c->stream); }))) return rc;
    if (bad) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_update_vertices: a vertex with a non-finite x, y or z (the scene is unchanged)");
    // motion (prt.h prt_set_motion): the records as they are go to the snapshot before the refit overwrites them -- unless one is pending
    // already: of several updates between two guide renders the oldest geometry is the one the motion plane is measured from.  Every
    // refusal is behind us (an allocation failure here still leaves the scene as it was)
    if (c->motion && !sn.snap.snap_valid) {
        HIPCHK(c, sn.snap.tri_prev.first_use(sn.n_slots));
        HIPCHK(c, hipMemcpyAsync(sn.snap.tri_prev, tree.tri_geom, (sn.n_slots ? sn.n_slots : 1) * sizeof(TriGeom), hipMemcpyDeviceToDevice, c->stream));
        sn.snap.snap_valid = true;
    }
    RefitTables t;
    t.slot_vtx = tree.slot_vtx; t.n_slots = sn.n_slots;
    t.level_pairs = tree.level_pairs;
    t.level_first = sn.level_first.data(); t.n_levels = sn.level_first.empty() ? 0u : (uint32_t)sn.level_first.size() - 1u;
    t.root_is_leaf = c->sc.root_is_leaf; t.root_leaf_first = c->sc.root_leaf_first; t.root_leaf_count = c->sc.root_leaf_count;
    // what a primary ray sees changes: the guides go stale and measured tile orders are forgotten, as with prt_set_camera; the path state,
    // the framebuffer and both histories stay (prt.h)
    c->frame.guides_valid = false;
    forget_tile_orders(c);
    sn.refitted = true;
    if (sn.smooth.on && !n) n = generate_normals(c, v);
    launch_refit(t, v, n, tree.pairs, tree.tri_geom, tree.tri_nrm, tree.root, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the caller's buffers may be reused on return
    return sn.policy.on ? policy_after_refit(c, d_vertices, d_normals) : PRT_OK;
}

extern "C" int prt_update_vertices(prt_ctx* c, const float* vertices, const float* normals) {
    CTX_CHECK(c);
    int rc = refit_prepare(c, vertices, "prt_update_vertices");
    if (!rc) rc = stage_vertices(c, vertices, normals);
    if (rc) return rc;
    return prt_update_vertices_device(c, c->scene.stage_vtx, normals ? c->scene.stage_nrm.get() : nullptr);
}

// ---- moving spheres, SDF primitives and quads: new prt_mesh records into the uploaded tables (prt.h prt_update_primitives; pt_prims.hip) --------
// the refusals both variants share; *nothing: count == 0 on a scene without primitives (the call succeeds and does nothing)
static int prims_checks(prt_ctx* c, const void* meshes, uint32_t count, const char* who, bool* nothing) {
    const std::string w(who);
    *nothing = false;
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, w + ": no scene uploaded");
    if (count != c->sc.n_meshes) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": count is not object_count[7] of the uploaded scene (the scene is unchanged)");
    if (count == 0) { *nothing = true; return PRT_OK; }
    if (!meshes) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": null meshes");
    return PRT_OK;
}

// what the first update allocates: the types table behind the flag word, and the staging tables
static int prims_tables(prt_ctx* c) {
    Scene& sn = c->scene;
    if (sn.prim_types) return PRT_OK;
    HIPCHK(c, sn.stage_spheres.first_use(c->sc.n_spheres));
    HIPCHK(c, sn.stage_sdfs.first_use(c->sc.n_sdfs));
    HIPCHK(c, sn.stage_quads.first_use(c->sc.n_quads));
    DevBuf<unsigned char> types;
    HIPCHK(c, types.alloc(16 + sn.mesh_t.size()));
    HIPCHK(c, hipMemcpy(types + 16, sn.mesh_t.data(), sn.mesh_t.size(), hipMemcpyHostToDevice));
    sn.prim_types = std::move(types);
    return PRT_OK;
}

extern "C" int prt_update_primitives_device(prt_ctx* c, const void* d_meshes, uint32_t count) {
    CTX_CHECK(c);
    bool nothing = false;
    if (int rc = prims_checks(c, d_meshes, count, "prt_update_primitives_device", &nothing)) return rc;
    if (nothing) return PRT_OK;
    if (!aligned16(d_meshes)) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_update_primitives_device: the device buffer must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = prims_tables(c)) return rc;
    Scene& sn = c->scene;
    Snapshots& snap = sn.snap;
    const size_t sph_bytes = c->sc.n_spheres * sizeof(DevSphere), sdf_bytes = c->sc.n_sdfs * sizeof(DevSdf), quad_bytes = c->sc.n_quads * sizeof(DevQuad);
    // the snapshot's tables before any refusal is decided: an allocation failure leaves the scene and a pending snapshot as they were
    if (c->motion && !snap.prim_snap_valid) {
        HIPCHK(c, snap.spheres_prev.first_use(c->sc.n_spheres));
        HIPCHK(c, snap.sdfs_prev.first_use(c->sc.n_sdfs));
        HIPCHK(c, snap.quads_prev.first_use(c->sc.n_quads));
    }
    // the pack and its check into the staging tables: the flag is read before anything live is overwritten
    uint32_t* flag = reinterpret_cast<uint32_t*>(sn.prim_types.get());
    uint32_t bad = 0;
    if (int rc = checked(c, flag, &bad, 1, [&] {
            launch_prims_pack(d_meshes, count, c->sc.n_spheres, c->sc.n_sdfs, sn.prim_types + 16, sn.stage_spheres, sn.stage_sdfs, sn.stage_quads, flag, c->stream);
        })) return rc;
    if (bad) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_update_primitives: a record whose t differs from the uploaded one, or a non-finite value in a field that is read (the scene is unchanged)");
    // motion (prt.h prt_set_motion): the tables as they are go to the snapshot before they are overwritten -- unless one is pending already:
    // the oldest wins.  Every refusal is behind us
    if (c->motion && !snap.prim_snap_valid) {
        if (sph_bytes) HIPCHK(c, hipMemcpyAsync(snap.spheres_prev, sn.spheres, sph_bytes, hipMemcpyDeviceToDevice, c->stream));
        if (sdf_bytes) HIPCHK(c, hipMemcpyAsync(snap.sdfs_prev, sn.sdfs, sdf_bytes, hipMemcpyDeviceToDevice, c->stream));
        if (quad_bytes) HIPCHK(c, hipMemcpyAsync(snap.quads_prev, sn.quads, quad_bytes, hipMemcpyDeviceToDevice, c->stream));
        snap.prim_snap_valid = true;
    }
    // what a primary ray sees changes: the lifetime of prt_update_vertices
    c->frame.guides_valid = false;
    forget_tile_orders(c);
    if (sph_bytes) HIPCHK(c, hipMemcpyAsync(sn.spheres, sn.stage_spheres, sph_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (sdf_bytes) HIPCHK(c, hipMemcpyAsync(sn.sdfs, sn.stage_sdfs, sdf_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (quad_bytes) HIPCHK(c, hipMemcpyAsync(sn.quads, sn.stage_quads, quad_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the caller's buffer may be reused on return
    return PRT_OK;
}

extern "C" int prt_update_primitives(prt_ctx* c, const prt_mesh* meshes, uint32_t count) {
    CTX_CHECK(c);
    bool nothing = false;
    if (int rc = prims_checks(c, meshes, count, "prt_update_primitives", &nothing)) return rc;
    if (nothing) return PRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->scene.stage_meshes.first_use(count));
    HIPCHK(c, hipMemcpyAsync(c->scene.stage_meshes, meshes, (size_t)count * sizeof(prt_mesh), hipMemcpyHostToDevice, c->stream));
    return prt_update_primitives_device(c, c->scene.stage_meshes, count);
}

// ---- the tree's read-backs (the caller has waited for the context's work: prt_synchronize) ---------------------------------------------------
// the first n records of a device buffer
template <typename T>
static hipError_t download(const DevBuf<T>& src, size_t n, std::vector<T>& out) {
    out.resize(n);
    return n ? hipMemcpy(out.data(), src, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

// the slot table of the current tree: the uploaded tree's is on the host, a rebuilt tree's on the device only -- that one comes into
// `scratch`.  Null: the copy failed (prt_last_error says how)
static const std::vector<uint32_t>* current_slot_vtx(prt_ctx* c, std::vector<uint32_t>& scratch) {
    if (!c->scene.rebuilt) return &c->scene.slot_vtx;
    const hipError_t e = download(c->scene.tree.slot_vtx, c->scene.n_slots, scratch);
    if (e != hipSuccess) c->err = std::string("the slot table of the rebuilt tree: ") + hipGetErrorString(e);
    return e == hipSuccess ? &scratch : nullptr;
}

extern "C" int prt_read_bvh_bounds(prt_ctx* c, float* bounds6) {
    CTX_CHECK(c);
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, "prt_read_bvh_bounds: no scene uploaded");
    if (!bounds6) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_bvh_bounds: null pointer");
    if (!c->scene.n_nodes) return PRT_OK;
    int rc = prt_synchronize(c);
    if (rc) return rc;
    std::vector<NodePair> pairs;
    HIPCHK(c, download(c->scene.tree.pairs, c->sc.n_pairs, pairs));
    for (uint32_t i = 0; i < c->scene.n_nodes; ++i) {
        float* o = bounds6 + 6 * (size_t)i;
        const uint32_t at = c->scene.rebuilt ? i - 1u : c->scene.node_box[i];          // (a rebuilt tree: the children of pair k are nodes 2k + 1 and 2k + 2; i = 0 wraps to "none")
        if (at == 0xFFFFFFFFu) { for (int j = 0; j < 6; ++j) o[j] = 0.0f; continue; }      // (a node no pair reaches)
        std::memcpy(o, pairs[at >> 1].b + 6 * (at & 1u), 6 * sizeof(float));
    }
    // the root: stored in no pair.  After an update the device's; before, the same union over the uploaded pair 0 (a leaf root: as uploaded)
    if (c->scene.refitted) HIPCHK(c, hipMemcpy(bounds6, c->scene.tree.root, 6 * sizeof(float), hipMemcpyDeviceToHost));
    else if (c->sc.root_is_leaf) std::memcpy(bounds6, c->scene.root_bounds, 6 * sizeof(float));
    else {
        RefitQuad q[3];
        std::memcpy(q, pairs[0].b, sizeof(q));
        const RefitBox r = refit_union(q);
        std::memcpy(bounds6, r.b, 6 * sizeof(float));
    }
    return PRT_OK;
}

// ---- a new tree over all T triangles, built on the device (prt.h prt_rebuild_bvh; pt_build.hip) ------------------------------------------------
// the refusals both variants share (the host variant's come before its upload)
static int rebuild_checks(prt_ctx* c, const void* vertices, uint32_t max_leaf) {
    if (!c->have_scene || c->scene.n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_rebuild_bvh: no scene with triangles uploaded");
    if (!vertices) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: null vertices");
    if (max_leaf > 64u) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: max_leaf above 64 (the scene is unchanged)");
    return PRT_OK;
}

extern "C" int prt_rebuild_bvh_device(prt_ctx* c, const void* d_vertices, const void* d_normals, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = rebuild_checks(c, d_vertices, max_leaf)) return rc;
    if (!aligned16(d_vertices) || !aligned16(d_normals))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh_device: the device buffers must be 16-byte aligned");
    if (!max_leaf) max_leaf = PT_BUILD_DEFAULT_LEAF;
    Scene& sn = c->scene;
    CtxBuffers& x = c->ctx;
    const uint32_t T = sn.n_tris;
    const bool leaf_root = T <= max_leaf;
    const bool generate = sn.smooth.on && d_normals == nullptr;    // (smooth normals: a normal for every corner, nothing to carry)
    const bool carry_nrm = d_normals == nullptr && !generate;
    // the new tables: one slot per triangle, and room for the T - 1 pairs of a tree of single-triangle leaves
    if (int rc = table_limits(c, "prt_rebuild_bvh", T, T > 1u ? T - 1u : 1u)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refit_tables(c);                             // (the slot table of the tree being replaced: "old slot of triangle")
    if (rc) return rc;
    // every allocation first: the scratch, and the spare set the new tree is built into
    if (!x.build || x.build_T != T) {
        BuildWork w{};
        size_t bytes = 0;
        HIPCHK(c, build_work_layout(T, nullptr, w, &bytes));
        x.build_T = 0;
        HIPCHK(c, x.build.alloc(bytes));
        HIPCHK(c, build_work_layout(T, x.build, x.bw, &bytes));
        x.build_T = T;
    }
    TreeSet& sp = x.spare;
    const size_t want_pairs = T > 1u ? T - 1u : 1u;
    HIPCHK(c, sp.pairs.reserve(want_pairs));
    HIPCHK(c, sp.level_pairs.reserve(want_pairs));
    HIPCHK(c, sp.tri_geom.reserve(T));
    HIPCHK(c, sp.tri_nrm.reserve(T));
    HIPCHK(c, sp.slot_vtx.reserve(T));
    HIPCHK(c, sp.root.first_use(8));
    if (c->motion) HIPCHK(c, x.spare_prev.reserve(T));
    const BuildWork& w = x.bw;
    const float* v = static_cast<const float*>(d_vertices);
    const float* n = static_cast<const float*>(d_normals);
    // the checks: nothing of the scene is written before their flags are read
    const bool need_old = carry_nrm || c->motion;
    uint32_t bad[4] = {0, 0, 0, 0};                       // [0], [1] of BuildWork::flags
    if ((rc = checked(c, w.flags, bad, 4, [&] {
            launch_refit_check(v, 3 * (size_t)T, w.flags, c->stream);
            if (need_old) launch_build_old_slots(w, sn.tree.slot_vtx, sn.n_slots, T, carry_nrm, c->stream);
        }))) return rc;
    if (bad[0]) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: a vertex with a non-finite x, y or z (the scene is unchanged)");
    if (bad[1]) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: normals == NULL, and the current tree holds no normals for some triangle (the scene is unchanged)");
    if (generate) n = generate_normals(c, v);
    // rules 1 - 7, then the one small copy the host needs
    HIPCHK(c, launch_build_tree(w, v, T, max_leaf, sp.pairs, sp.slot_vtx, sp.level_pairs, c->stream));
    BuildHeader h;
    HIPCHK(c, hipMemcpyAsync(&h, w.hdr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(sp.root, 0, 32, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!leaf_root && (h.n_pairs == 0 || h.n_pairs > T - 1u || h.n_levels == 0 || h.n_levels > 64u || h.level_first[h.n_levels] != h.n_pairs))
        return fail(c, PRT_ERR_HIP, "prt_rebuild_bvh: the build left an inconsistent header (the scene is unchanged)");
    std::vector<uint32_t> level_first;
    if (!leaf_root) level_first.assign(h.level_first, h.level_first + h.n_levels + 1u);
    // rule 8: the records and the boxes by the refit's own kernels over the new tables
    RefitTables t;
    t.slot_vtx = sp.slot_vtx; t.n_slots = T;
    t.level_pairs = sp.level_pairs;
    t.level_first = level_first.data(); t.n_levels = leaf_root ? 0u : h.n_levels;
    t.root_is_leaf = leaf_root ? 1 : 0; t.root_leaf_first = 0; t.root_leaf_count = leaf_root ? T : 0u;
    launch_refit(t, v, n, sp.pairs, sp.tri_geom, sp.tri_nrm, sp.root, c->stream);
    // what is carried to the new slot order: the normals (normals == NULL) and the motion snapshot -- a pending one, else the records as they are
    if (need_old) {
        const TriGeom* prev_old = sn.snap.snap_valid && sn.snap.tri_prev ? sn.snap.tri_prev : sn.tree.tri_geom;
        launch_build_carry(w, sp.slot_vtx, T, carry_nrm, sn.tree.tri_nrm, sp.tri_nrm, prev_old, sp.tri_geom, c->motion ? x.spare_prev.get() : nullptr, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));         // the caller's buffers may be reused on return; nothing reads the old set any more
    // the swap: from here on the scene is the new tree
    std::swap(sn.tree, sp);
    if (c->motion) { sn.snap.tri_prev.swap(x.spare_prev); sn.snap.snap_valid = true; }
    bind(c);
    c->sc.n_pairs = leaf_root ? 0u : h.n_pairs;
    c->sc.stack_levels = leaf_root ? 1u : h.max_two + 1u;
    c->sc.root_is_leaf = leaf_root ? 1 : 0;
    c->sc.root_leaf_first = 0; c->sc.root_leaf_count = leaf_root ? T : 0u;
    sn.level_first.swap(level_first);
    sn.slot_vtx.clear(); sn.level_pairs.clear(); sn.node_box.clear();
    sn.n_slots = T;
    sn.n_nodes = 2u * c->sc.n_pairs + 1u;
    sn.rebuilt = sn.refit_ready = sn.refitted = true;
    c->frame.guides_valid = false;
    forget_tile_orders(c);
    return sn.policy.on ? measure_cost(c, &sn.policy.baseline) : PRT_OK;       // (prt_set_rebuild_policy: every accepted rebuild moves the baseline)
}

extern "C" int prt_rebuild_bvh(prt_ctx* c, const float* vertices, const float* normals, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = rebuild_checks(c, vertices, max_leaf)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = stage_vertices(c, vertices, normals)) return rc;
    return prt_rebuild_bvh_device(c, c->scene.stage_vtx, normals ? c->scene.stage_nrm.get() : nullptr, max_leaf);
}

extern "C" int prt_read_bvh(prt_ctx* c, prt_bvh_node* nodes, uint32_t* node_count, uint64_t* primitive_indices) {
    CTX_CHECK(c);
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, "prt_read_bvh: no scene uploaded");
    if (node_count) *node_count = c->scene.n_nodes;
    if (!c->scene.n_nodes || (!nodes && !primitive_indices)) return PRT_OK;
    if (!c->scene.rebuilt) {
        // the uploaded tree with the current boxes (a node no inner node names as a child keeps the box it came with)
        if (primitive_indices) std::memcpy(primitive_indices, c->scene.up_prims.data(), c->scene.up_prims.size() * sizeof(uint64_t));
        if (!nodes) return PRT_OK;
        std::vector<float> b(6 * (size_t)c->scene.n_nodes);
        int rc = prt_read_bvh_bounds(c, b.data());
        if (rc) return rc;
        for (uint32_t i = 0; i < c->scene.n_nodes; ++i) {
            nodes[i] = c->scene.up_nodes[i];
            if (i == 0 || c->scene.node_box[i] != 0xFFFFFFFFu) std::memcpy(nodes[i].bounds, b.data() + 6 * (size_t)i, 6 * sizeof(float));
        }
        return PRT_OK;
    }
    int rc = prt_synchronize(c);
    if (rc) return rc;
    if (primitive_indices) {
        std::vector<uint32_t> scratch;
        const std::vector<uint32_t>* sv = current_slot_vtx(c, scratch);
        if (!sv) return PRT_ERR_HIP;
        for (size_t s = 0; s < sv->size(); ++s) primitive_indices[s] = (*sv)[s] / 3u;
    }
    if (!nodes) return PRT_OK;
    std::vector<NodePair> pairs;
    HIPCHK(c, download(c->scene.tree.pairs, c->sc.n_pairs, pairs));
    std::memset(nodes, 0, sizeof(prt_bvh_node) * (size_t)c->scene.n_nodes);
    HIPCHK(c, hipMemcpy(nodes[0].bounds, c->scene.tree.root, 6 * sizeof(float), hipMemcpyDeviceToHost));
    if (c->sc.root_is_leaf) {
        nodes[0].first_child_or_primitive = c->sc.root_leaf_first; nodes[0].primitive_count = c->sc.root_leaf_count; nodes[0].is_leaf = 1;
        return PRT_OK;
    }
    nodes[0].first_child_or_primitive = 1;
    for (uint32_t k = 0; k < c->sc.n_pairs; ++k)
        for (uint32_t ch = 0; ch < 2; ++ch) {
            prt_bvh_node& nd = nodes[2 * k + 1 + ch];
            std::memcpy(nd.bounds, pairs[k].b + 6 * ch, 6 * sizeof(float));
            if (pairs[k].meta[2 * ch + 1] == 0xFFFFFFFFu) nd.first_child_or_primitive = 2u * pairs[k].meta[2 * ch] + 1u;
            else { nd.first_child_or_primitive = pairs[k].meta[2 * ch]; nd.primitive_count = pairs[k].meta[2 * ch + 1]; nd.is_leaf = 1; }
        }
    return PRT_OK;
}

// ---- motion of deforming geometry (prt.h prt_set_motion) ---------------------------------------------------------------------------------------
extern "C" int prt_set_motion(prt_ctx* c, int enable) {
    CTX_CHECK(c);
    if (enable && c->cfg.view_option != PRT_VIEW_RESULTS) return fail(c, PRT_ERR_UNSUPPORTED, "prt_set_motion: a debug view has no denoiser to carry motion into");
    if ((enable != 0) == c->motion) return PRT_OK;     // (unchanged: a per-frame call costs nothing and keeps the guides)
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->motion = enable != 0;
    c->frame.guides_valid = false;                           // (both histories are kept, as by prt_set_camera)
    c->frame.motion_valid = false;
    if (!c->motion) c->scene.snap = Snapshots{};
    return PRT_OK;
}

extern "C" int prt_read_normals(prt_ctx* c, float* normals) {
    CTX_CHECK(c);
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, "prt_read_normals: no scene uploaded");
    if (!normals) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_normals: null pointer");
    const size_t T = c->scene.n_tris;
    if (!T) return PRT_OK;
    std::memset(normals, 0, 3 * T * 4 * sizeof(float));
    if (!c->scene.n_slots) return PRT_OK;
    int rc = prt_synchronize(c);
    if (rc) return rc;
    std::vector<uint32_t> scratch;
    const std::vector<uint32_t>* sv = current_slot_vtx(c, scratch);
    if (!sv) return PRT_ERR_HIP;
    const std::vector<uint32_t>& slot_vtx = *sv;
    std::vector<TriNrm> tn;
    HIPCHK(c, download(c->scene.tree.tri_nrm, c->scene.n_slots, tn));
    for (size_t s = 0; s < slot_vtx.size() && s < tn.size(); ++s) {
        const size_t fv = slot_vtx[s];
        if (fv + 3 > 3 * T) continue;
        const float* rec = reinterpret_cast<const float*>(&tn[s]);
        for (int k = 0; k < 3; ++k) {
            float* o = normals + 4 * (fv + k);
            o[0] = rec[4 * k]; o[1] = rec[4 * k + 1]; o[2] = rec[4 * k + 2]; o[3] = 0.0f;
        }
    }
    return PRT_OK;
}
