// prt_api_scene.cpp -- the scene calls of the C ABI (include/prt.h): upload, vertex updates with a refit, rebuilds, the tree's read-backs,
// motion on / off, smooth normals.
#include <cmath>
#include <new>
#include <utility>

#include "prt_ctx.h"
#include "pt_build.h"
#include "pt_normals.h"
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
    // from here on the old buffers are being replaced: the context has no scene until every upload has succeeded
    c->have_scene = false;
    c->guides_valid = false;
    c->hist.valid = false;
    // (the refit tables and staging buffers are the old tree's: a static scene holds none on the device)
    free_dev(c->d_slot_vtx); free_dev(c->d_level_pairs); free_dev(c->d_refit_root); free_dev(c->d_stage_vtx); free_dev(c->d_stage_nrm);
    c->refit_ready = c->refitted = false;
    free_dev(c->d_tri_prev);                         // (the snapshot is the old scene's: no motion across an upload)
    c->snap_valid = false;
    c->cap_prev = 0;
    c->rebuilt = false;
    free_smooth(c);                                  // (the smoothing topology is the old mesh's: T may have changed)
    free_prims(c, true);                             // (the primitive snapshot, types and staging tables are the old scene's)
    c->mesh_t.resize(s->object_count[7]);
    for (uint32_t i = 0; i < s->object_count[7]; ++i) c->mesh_t[i] = s->meshes[i].t;
    c->n_slots = ps.slot_vtx.size();
    c->cap_pairs = ps.pairs.empty() ? 1 : ps.pairs.size();         // (what upload() below allocates, in records)
    c->cap_slots = ps.tg.empty() ? 1 : ps.tg.size();
    if (s->triangle_count) {
        c->up_nodes.assign(s->bvh_nodes, s->bvh_nodes + s->bvh_node_count);
        c->up_prims.assign(s->primitive_indices, s->primitive_indices + s->triangle_count);
    } else { c->up_nodes.clear(); c->up_prims.clear(); }
    c->slot_vtx.swap(ps.slot_vtx); c->level_pairs.swap(ps.level_pairs); c->level_first.swap(ps.level_first); c->node_box.swap(ps.node_box);
    std::memcpy(c->root_bounds, ps.root_bounds, sizeof(c->root_bounds));
    c->n_tris = s->triangle_count; c->n_nodes = s->triangle_count ? s->bvh_node_count : 0u;
    const float* env = c->sc.env; const int env_w = c->sc.env_w, env_h = c->sc.env_h;    // the environment map survives scene uploads
    const float* env_rows = c->sc.env_cdf_rows; const float* env_cols = c->sc.env_cdf_cols;
    c->sc = DevScene{};
    c->sc.env = env; c->sc.env_w = env_w; c->sc.env_h = env_h; c->sc.env_cdf_rows = env_rows; c->sc.env_cdf_cols = env_cols;
    if ((rc = upload(c, c->d_pairs, ps.pairs)) || (rc = upload(c, c->d_tri_geom, ps.tg)) || (rc = upload(c, c->d_tri_nrm, ps.tn)) ||
        (rc = upload(c, c->d_spheres, ps.spheres)) || (rc = upload(c, c->d_quads, ps.quads)) || (rc = upload(c, c->d_sdfs, ps.sdfs)) ||
        (rc = upload(c, c->d_mats, ps.mats)) || (rc = upload(c, c->d_light_tab, ps.light_tab)))
        return rc;
    DevScene sc = ps.sc;
    sc.pairs = static_cast<const NodePair*>(c->d_pairs);
    sc.tri_geom = static_cast<const TriGeom*>(c->d_tri_geom);
    sc.tri_nrm = static_cast<const TriNrm*>(c->d_tri_nrm);
    sc.spheres = static_cast<const DevSphere*>(c->d_spheres);
    sc.quads = static_cast<const DevQuad*>(c->d_quads);
    sc.sdfs = static_cast<const DevSdf*>(c->d_sdfs);
    sc.mats = static_cast<const DevMaterial*>(c->d_mats);
    sc.light_tab = static_cast<const uint32_t*>(c->d_light_tab);
    sc.env = env; sc.env_w = env_w; sc.env_h = env_h; sc.env_cdf_rows = env_rows; sc.env_cdf_cols = env_cols;
    c->sc = sc;
    if (!c->sc.env) {
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
    if (!c->have_scene || c->n_tris == 0) return fail(c, PRT_ERR_NOT_READY, w + ": no scene with triangles uploaded");
    if (!vertices) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": null vertices");
    if (!c->sc.root_is_leaf && c->level_first.size() > 257u)
        return fail(c, PRT_ERR_UNSUPPORTED, w + ": the tree has more than 256 levels of pairs (one launch per level)");
    if (int rc = table_limits(c, w, c->n_slots, c->sc.n_pairs)) return rc;       // (the tables the refit kernels write)
    HIPCHK(c, hipSetDevice(c->device));
    return refit_tables(c);
}

// the tables of the uploaded tree on the device (a rebuilt tree's are there from its build)
int refit_tables(prt_ctx* c) {
    if (!c->refit_ready) {
        int rc;
        if ((rc = upload(c, c->d_slot_vtx, c->slot_vtx)) || (rc = upload(c, c->d_level_pairs, c->level_pairs))) return rc;
        free_dev(c->d_refit_root);
        HIPCHK(c, hipMalloc(&c->d_refit_root, 32));
        float init[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        std::memcpy(init, c->root_bounds, sizeof(c->root_bounds));      // (an empty leaf root keeps the box it was uploaded with)
        HIPCHK(c, hipMemcpy(c->d_refit_root, init, sizeof(init), hipMemcpyHostToDevice));
        c->refit_ready = true;
    }
    return PRT_OK;
}

// the host variants' vertices (and normals, unless null) into the staging buffers on the context's stream
static int stage_vertices(prt_ctx* c, const float* vertices, const float* normals) {
    const size_t bytes = 3 * (size_t)c->n_tris * 16;
    if (!c->d_stage_vtx) HIPCHK(c, hipMalloc(&c->d_stage_vtx, bytes));
    if (normals && !c->d_stage_nrm) HIPCHK(c, hipMalloc(&c->d_stage_nrm, bytes));
    HIPCHK(c, hipMemcpyAsync(c->d_stage_vtx, vertices, bytes, hipMemcpyHostToDevice, c->stream));
    if (normals) HIPCHK(c, hipMemcpyAsync(c->d_stage_nrm, normals, bytes, hipMemcpyHostToDevice, c->stream));
    return PRT_OK;
}

// smooth normals on and no normals given (prt.h prt_set_smooth_normals): the normals of the new vertices into the context's own buffer, two
// launches on the context's stream; the caller passes the buffer on as if it had been given.  Called once the finite-vertex check has passed:
// only scratch of the context is written
static const float* generate_normals(prt_ctx* c, const float* v) {
    SmoothTables t;
    t.corner_group = static_cast<const uint32_t*>(c->d_sm_group); t.group_first = static_cast<const uint32_t*>(c->d_sm_first);
    t.member_face = static_cast<const uint32_t*>(c->d_sm_member);
    t.face_f = c->d_sm_face_f; t.face_r = c->smooth_weighting == PRT_NORMALS_AREA ? c->d_sm_face_r : nullptr;
    t.n_tris = c->n_tris; t.crease_cos = c->smooth_crease;
    launch_smooth_normals(t, v, static_cast<float*>(c->d_sm_nrm), c->stream);
    return static_cast<const float*>(c->d_sm_nrm);
}

extern "C" int prt_update_vertices_device(prt_ctx* c, const void* d_vertices, const void* d_normals) {
    CTX_CHECK(c);
    int rc = refit_prepare(c, d_vertices, "prt_update_vertices_device");
    if (rc) return rc;
    if (!aligned16(d_vertices) || !aligned16(d_normals))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_update_vertices_device: the device buffers must be 16-byte aligned");
    const float* v = static_cast<const float*>(d_vertices);
    const float* n = static_cast<const float*>(d_normals);
    uint32_t* flag = static_cast<uint32_t*>(c->d_refit_root) + 6;
    // the check first: its flag is read before anything of the scene is overwritten
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(uint32_t), c->stream));
    launch_refit_check(v, 3 * (size_t)c->n_tris, flag, c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_update_vertices: a vertex with a non-finite x, y or z (the scene is unchanged)");
    // motion (prt.h prt_set_motion): the records as they are go to the snapshot before the refit overwrites them -- unless one is pending
    // already: of several updates between two guide renders the oldest geometry is the one the motion plane is measured from.  Every
    // refusal is behind us (an allocation failure here still leaves the scene as it was)
    if (c->motion && !c->snap_valid) {
        const size_t snap_bytes = (c->n_slots ? c->n_slots : 1) * sizeof(TriGeom);
        if (!c->d_tri_prev) { HIPCHK(c, hipMalloc(&c->d_tri_prev, snap_bytes)); c->cap_prev = c->n_slots ? c->n_slots : 1; }
        HIPCHK(c, hipMemcpyAsync(c->d_tri_prev, c->d_tri_geom, snap_bytes, hipMemcpyDeviceToDevice, c->stream));
        c->snap_valid = true;
    }
    RefitTables t;
    t.slot_vtx = static_cast<const uint32_t*>(c->d_slot_vtx); t.n_slots = c->n_slots;
    t.level_pairs = static_cast<const uint32_t*>(c->d_level_pairs);
    t.level_first = c->level_first.data(); t.n_levels = c->level_first.empty() ? 0u : (uint32_t)c->level_first.size() - 1u;
    t.root_is_leaf = c->sc.root_is_leaf; t.root_leaf_first = c->sc.root_leaf_first; t.root_leaf_count = c->sc.root_leaf_count;
    // what a primary ray sees changes: the guides go stale and measured tile orders are forgotten, as with prt_set_camera; the path state,
    // the framebuffer and both histories stay (prt.h)
    c->guides_valid = false;
    forget_tile_orders(c);
    c->refitted = true;
    if (c->smooth && !n) n = generate_normals(c, v);
    launch_refit(t, v, n, static_cast<NodePair*>(c->d_pairs), static_cast<TriGeom*>(c->d_tri_geom), static_cast<TriNrm*>(c->d_tri_nrm),
                 static_cast<float*>(c->d_refit_root), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the caller's buffers may be reused on return
    return PRT_OK;
}

extern "C" int prt_update_vertices(prt_ctx* c, const float* vertices, const float* normals) {
    CTX_CHECK(c);
    int rc = refit_prepare(c, vertices, "prt_update_vertices");
    if (!rc) rc = stage_vertices(c, vertices, normals);
    if (rc) return rc;
    return prt_update_vertices_device(c, c->d_stage_vtx, normals ? c->d_stage_nrm : nullptr);
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
    if (c->d_prim_types) return PRT_OK;
    const size_t n_sph = c->sc.n_spheres ? c->sc.n_spheres : 1, n_sdf = c->sc.n_sdfs ? c->sc.n_sdfs : 1, n_quad = c->sc.n_quads ? c->sc.n_quads : 1;
    if (!c->d_stage_spheres) HIPCHK(c, hipMalloc(&c->d_stage_spheres, n_sph * sizeof(DevSphere)));
    if (!c->d_stage_sdfs) HIPCHK(c, hipMalloc(&c->d_stage_sdfs, n_sdf * sizeof(DevSdf)));
    if (!c->d_stage_quads) HIPCHK(c, hipMalloc(&c->d_stage_quads, n_quad * sizeof(DevQuad)));
    void* types = nullptr;
    HIPCHK(c, hipMalloc(&types, 16 + c->mesh_t.size()));
    hipError_t e = hipMemcpy(static_cast<char*>(types) + 16, c->mesh_t.data(), c->mesh_t.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { free_dev(types); HIPCHK(c, e); }
    c->d_prim_types = types;
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
    const size_t sph_bytes = c->sc.n_spheres * sizeof(DevSphere), sdf_bytes = c->sc.n_sdfs * sizeof(DevSdf), quad_bytes = c->sc.n_quads * sizeof(DevQuad);
    // the snapshot's tables before any refusal is decided: an allocation failure leaves the scene and a pending snapshot as they were
    if (c->motion && !c->prim_snap_valid) {
        if (!c->d_spheres_prev) HIPCHK(c, hipMalloc(&c->d_spheres_prev, sph_bytes ? sph_bytes : sizeof(DevSphere)));
        if (!c->d_sdfs_prev) HIPCHK(c, hipMalloc(&c->d_sdfs_prev, sdf_bytes ? sdf_bytes : sizeof(DevSdf)));
        if (!c->d_quads_prev) HIPCHK(c, hipMalloc(&c->d_quads_prev, quad_bytes ? quad_bytes : sizeof(DevQuad)));
    }
    // the pack and its check into the staging tables: the flag is read before anything live is overwritten
    uint32_t* flag = static_cast<uint32_t*>(c->d_prim_types);
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(uint32_t), c->stream));
    launch_prims_pack(d_meshes, count, c->sc.n_spheres, c->sc.n_sdfs, static_cast<const uint8_t*>(c->d_prim_types) + 16,
                      static_cast<DevSphere*>(c->d_stage_spheres), static_cast<DevSdf*>(c->d_stage_sdfs), static_cast<DevQuad*>(c->d_stage_quads), flag,
                      c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_update_primitives: a record whose t differs from the uploaded one, or a non-finite value in a field that is read (the scene is unchanged)");
    // motion (prt.h prt_set_motion): the tables as they are go to the snapshot before they are overwritten -- unless one is pending already:
    // the oldest wins.  Every refusal is behind us
    if (c->motion && !c->prim_snap_valid) {
        if (sph_bytes) HIPCHK(c, hipMemcpyAsync(c->d_spheres_prev, c->d_spheres, sph_bytes, hipMemcpyDeviceToDevice, c->stream));
        if (sdf_bytes) HIPCHK(c, hipMemcpyAsync(c->d_sdfs_prev, c->d_sdfs, sdf_bytes, hipMemcpyDeviceToDevice, c->stream));
        if (quad_bytes) HIPCHK(c, hipMemcpyAsync(c->d_quads_prev, c->d_quads, quad_bytes, hipMemcpyDeviceToDevice, c->stream));
        c->prim_snap_valid = true;
    }
    // what a primary ray sees changes: the lifetime of prt_update_vertices
    c->guides_valid = false;
    forget_tile_orders(c);
    if (sph_bytes) HIPCHK(c, hipMemcpyAsync(c->d_spheres, c->d_stage_spheres, sph_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (sdf_bytes) HIPCHK(c, hipMemcpyAsync(c->d_sdfs, c->d_stage_sdfs, sdf_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (quad_bytes) HIPCHK(c, hipMemcpyAsync(c->d_quads, c->d_stage_quads, quad_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the caller's buffer may be reused on return
    return PRT_OK;
}

extern "C" int prt_update_primitives(prt_ctx* c, const prt_mesh* meshes, uint32_t count) {
    CTX_CHECK(c);
    bool nothing = false;
    if (int rc = prims_checks(c, meshes, count, "prt_update_primitives", &nothing)) return rc;
    if (nothing) return PRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)count * sizeof(prt_mesh);
    if (!c->d_stage_meshes) HIPCHK(c, hipMalloc(&c->d_stage_meshes, bytes));
    HIPCHK(c, hipMemcpyAsync(c->d_stage_meshes, meshes, bytes, hipMemcpyHostToDevice, c->stream));
    return prt_update_primitives_device(c, c->d_stage_meshes, count);
}

extern "C" int prt_read_bvh_bounds(prt_ctx* c, float* bounds6) {
    CTX_CHECK(c);
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, "prt_read_bvh_bounds: no scene uploaded");
    if (!bounds6) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_bvh_bounds: null pointer");
    if (!c->n_nodes) return PRT_OK;
    int rc = prt_synchronize(c);
    if (rc) return rc;
    std::vector<NodePair> pairs(c->sc.n_pairs);
    if (!pairs.empty()) HIPCHK(c, hipMemcpy(pairs.data(), c->d_pairs, pairs.size() * sizeof(NodePair), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < c->n_nodes; ++i) {
        float* o = bounds6 + 6 * (size_t)i;
        const uint32_t at = c->rebuilt ? i - 1u : c->node_box[i];          // (a rebuilt tree: the children of pair k are nodes 2k + 1 and 2k + 2; i = 0 wraps to "none")
        if (at == 0xFFFFFFFFu) { for (int j = 0; j < 6; ++j) o[j] = 0.0f; continue; }      // (a node no pair reaches)
        std::memcpy(o, pairs[at >> 1].b + 6 * (at & 1u), 6 * sizeof(float));
    }
    // the root: stored in no pair.  After an update the device's; before, the same union over the uploaded pair 0 (a leaf root: as uploaded)
    if (c->refitted) HIPCHK(c, hipMemcpy(bounds6, c->d_refit_root, 6 * sizeof(float), hipMemcpyDeviceToHost));
    else if (c->sc.root_is_leaf) std::memcpy(bounds6, c->root_bounds, 6 * sizeof(float));
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
    if (!c->have_scene || c->n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_rebuild_bvh: no scene with triangles uploaded");
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
    const uint32_t T = c->n_tris;
    const bool leaf_root = T <= max_leaf;
    const bool generate = c->smooth && d_normals == nullptr;       // (smooth normals: a normal for every corner, nothing to carry)
    const bool carry_nrm = d_normals == nullptr && !generate;
    // the new tables: one slot per triangle, and room for the T - 1 pairs of a tree of single-triangle leaves
    if (int rc = table_limits(c, "prt_rebuild_bvh", T, T > 1u ? T - 1u : 1u)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refit_tables(c);                             // (the slot table of the tree being replaced: "old slot of triangle")
    if (rc) return rc;
    // every allocation first: the scratch, and the spare set the new tree is built into
    if (!c->d_build || c->build_T != T) {
        BuildWork w{};
        size_t bytes = 0;
        HIPCHK(c, build_work_layout(T, nullptr, w, &bytes));
        free_dev(c->d_build);
        c->build_T = 0;
        HIPCHK(c, hipMalloc(&c->d_build, bytes));
        HIPCHK(c, build_work_layout(T, c->d_build, c->bw, &bytes));
        c->build_T = T;
    }
    prt_ctx::TreeSet& sp = c->spare;
    const size_t want_pairs = T > 1u ? T - 1u : 1u;
    if (sp.cap_pairs < want_pairs) {                      // (pairs and level_pairs are sized alike)
        free_dev(sp.pairs); free_dev(sp.level_pairs);
        sp.cap_pairs = 0;
        HIPCHK(c, hipMalloc(&sp.pairs, want_pairs * sizeof(NodePair)));
        HIPCHK(c, hipMalloc(&sp.level_pairs, want_pairs * sizeof(uint32_t)));
        sp.cap_pairs = want_pairs;
    }
    if (sp.cap_slots < T) {                               // (the records and slot_vtx are sized alike: one slot per triangle)
        free_dev(sp.tri_geom); free_dev(sp.tri_nrm); free_dev(sp.slot_vtx);
        sp.cap_slots = 0;
        HIPCHK(c, hipMalloc(&sp.tri_geom, T * sizeof(TriGeom)));
        HIPCHK(c, hipMalloc(&sp.tri_nrm, T * sizeof(TriNrm)));
        HIPCHK(c, hipMalloc(&sp.slot_vtx, T * sizeof(uint32_t)));
        sp.cap_slots = T;
    }
    if (!sp.root) HIPCHK(c, hipMalloc(&sp.root, 32));
    if (c->motion && sp.cap_prev < T) {
        free_dev(sp.tri_prev);
        sp.cap_prev = 0;
        HIPCHK(c, hipMalloc(&sp.tri_prev, T * sizeof(TriGeom)));
        sp.cap_prev = T;
    }
    const BuildWork& w = c->bw;
    const float* v = static_cast<const float*>(d_vertices);
    const float* n = static_cast<const float*>(d_normals);
    // the checks: nothing of the scene is written before their flags are read
    HIPCHK(c, hipMemsetAsync(w.flags, 0, 16, c->stream));
    launch_refit_check(v, 3 * (size_t)T, w.flags, c->stream);
    const bool need_old = carry_nrm || c->motion;
    if (need_old) launch_build_old_slots(w, static_cast<const uint32_t*>(c->d_slot_vtx), c->n_slots, T, carry_nrm, c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t bad[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(bad, w.flags, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad[0]) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: a vertex with a non-finite x, y or z (the scene is unchanged)");
    if (bad[1]) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: normals == NULL, and the current tree holds no normals for some triangle (the scene is unchanged)");
    if (generate) n = generate_normals(c, v);
    // rules 1 - 7, then the one small copy the host needs
    HIPCHK(c, launch_build_tree(w, v, T, max_leaf, static_cast<NodePair*>(sp.pairs), static_cast<uint32_t*>(sp.slot_vtx), static_cast<uint32_t*>(sp.level_pairs), c->stream));
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
    t.slot_vtx = static_cast<const uint32_t*>(sp.slot_vtx); t.n_slots = T;
    t.level_pairs = static_cast<const uint32_t*>(sp.level_pairs);
    t.level_first = level_first.data(); t.n_levels = leaf_root ? 0u : h.n_levels;
    t.root_is_leaf = leaf_root ? 1 : 0; t.root_leaf_first = 0; t.root_leaf_count = leaf_root ? T : 0u;
    launch_refit(t, v, n, static_cast<NodePair*>(sp.pairs), static_cast<TriGeom*>(sp.tri_geom), static_cast<TriNrm*>(sp.tri_nrm), static_cast<float*>(sp.root), c->stream);
    // what is carried to the new slot order: the normals (normals == NULL) and the motion snapshot -- a pending one, else the records as they are
    if (need_old) {
        const TriGeom* prev_old = static_cast<const TriGeom*>(c->snap_valid && c->d_tri_prev ? c->d_tri_prev : c->d_tri_geom);
        launch_build_carry(w, static_cast<const uint32_t*>(sp.slot_vtx), T, carry_nrm, static_cast<const TriNrm*>(c->d_tri_nrm), static_cast<TriNrm*>(sp.tri_nrm),
                           prev_old, static_cast<const TriGeom*>(sp.tri_geom), c->motion ? static_cast<TriGeom*>(sp.tri_prev) : nullptr, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));         // the caller's buffers may be reused on return; nothing reads the old set any more
    // the swap: from here on the scene is the new tree
    std::swap(c->d_pairs, sp.pairs); std::swap(c->d_tri_geom, sp.tri_geom); std::swap(c->d_tri_nrm, sp.tri_nrm);
    std::swap(c->d_slot_vtx, sp.slot_vtx); std::swap(c->d_level_pairs, sp.level_pairs); std::swap(c->d_refit_root, sp.root);
    std::swap(c->cap_pairs, sp.cap_pairs); std::swap(c->cap_slots, sp.cap_slots);
    if (c->motion) { std::swap(c->d_tri_prev, sp.tri_prev); std::swap(c->cap_prev, sp.cap_prev); c->snap_valid = true; }
    c->sc.pairs = static_cast<const NodePair*>(c->d_pairs);
    c->sc.tri_geom = static_cast<const TriGeom*>(c->d_tri_geom);
    c->sc.tri_nrm = static_cast<const TriNrm*>(c->d_tri_nrm);
    c->sc.n_pairs = leaf_root ? 0u : h.n_pairs;
    c->sc.stack_levels = leaf_root ? 1u : h.max_two + 1u;
    c->sc.root_is_leaf = leaf_root ? 1 : 0;
    c->sc.root_leaf_first = 0; c->sc.root_leaf_count = leaf_root ? T : 0u;
    c->level_first.swap(level_first);
    c->slot_vtx.clear(); c->level_pairs.clear(); c->node_box.clear();
    c->n_slots = T;
    c->n_nodes = 2u * c->sc.n_pairs + 1u;
    c->rebuilt = c->refit_ready = c->refitted = true;
    c->guides_valid = false;
    forget_tile_orders(c);
    return PRT_OK;
}

extern "C" int prt_rebuild_bvh(prt_ctx* c, const float* vertices, const float* normals, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (int rc = rebuild_checks(c, vertices, max_leaf)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = stage_vertices(c, vertices, normals)) return rc;
    return prt_rebuild_bvh_device(c, c->d_stage_vtx, normals ? c->d_stage_nrm : nullptr, max_leaf);
}

extern "C" int prt_read_bvh(prt_ctx* c, prt_bvh_node* nodes, uint32_t* node_count, uint64_t* primitive_indices) {
    CTX_CHECK(c);
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, "prt_read_bvh: no scene uploaded");
    if (node_count) *node_count = c->n_nodes;
    if (!c->n_nodes || (!nodes && !primitive_indices)) return PRT_OK;
    if (!c->rebuilt) {
        // the uploaded tree with the current boxes (a node no inner node names as a child keeps the box it came with)
        if (primitive_indices) std::memcpy(primitive_indices, c->up_prims.data(), c->up_prims.size() * sizeof(uint64_t));
        if (!nodes) return PRT_OK;
        std::vector<float> b(6 * (size_t)c->n_nodes);
        int rc = prt_read_bvh_bounds(c, b.data());
        if (rc) return rc;
        for (uint32_t i = 0; i < c->n_nodes; ++i) {
            nodes[i] = c->up_nodes[i];
            if (i == 0 || c->node_box[i] != 0xFFFFFFFFu) std::memcpy(nodes[i].bounds, b.data() + 6 * (size_t)i, 6 * sizeof(float));
        }
        return PRT_OK;
    }
    int rc = prt_synchronize(c);
    if (rc) return rc;
    if (primitive_indices) {
        std::vector<uint32_t> sv(c->n_slots);
        HIPCHK(c, hipMemcpy(sv.data(), c->d_slot_vtx, sv.size() * 4, hipMemcpyDeviceToHost));
        for (size_t s = 0; s < sv.size(); ++s) primitive_indices[s] = sv[s] / 3u;
    }
    if (!nodes) return PRT_OK;
    std::vector<NodePair> pairs(c->sc.n_pairs);
    if (!pairs.empty()) HIPCHK(c, hipMemcpy(pairs.data(), c->d_pairs, pairs.size() * sizeof(NodePair), hipMemcpyDeviceToHost));
    std::memset(nodes, 0, sizeof(prt_bvh_node) * (size_t)c->n_nodes);
    HIPCHK(c, hipMemcpy(nodes[0].bounds, c->d_refit_root, 6 * sizeof(float), hipMemcpyDeviceToHost));
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
    c->guides_valid = false;                           // (both histories are kept, as by prt_set_camera)
    c->motion_valid = false;
    if (!c->motion) {
        free_dev(c->d_tri_prev);
        c->cap_prev = 0;
        c->snap_valid = false;
        free_prims(c, false);
    }
    return PRT_OK;
}

// ---- smooth shading normals regenerated from new vertices (prt.h prt_set_smooth_normals; pt_normals.hip) ---------------------------------------
extern "C" int prt_set_smooth_normals(prt_ctx* c, const uint32_t* corner_group, uint32_t n_groups, uint32_t weighting, float crease_cos) {
    CTX_CHECK(c);
    if (!c->have_scene || c->n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_set_smooth_normals: no scene with triangles uploaded");
    HIPCHK(c, hipSetDevice(c->device));
    if (!corner_group) {                                   // off: nothing of the scene changes, the buffers go
        HIPCHK(c, hipStreamSynchronize(c->stream));
        free_smooth(c);
        return PRT_OK;
    }
    // every refusal before anything of the topology in force is touched
    if (n_groups == 0) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_smooth_normals: n_groups is 0 (the topology in force stays)");
    if (weighting != PRT_NORMALS_UNIT && weighting != PRT_NORMALS_AREA)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_smooth_normals: unknown weighting (the topology in force stays)");
    if (!std::isfinite(crease_cos)) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_smooth_normals: crease_cos is not finite (the topology in force stays)");
    const uint32_t T = c->n_tris;
    if (T > PRT_MAX_TRIANGLE_SLOTS)
        return fail(c, PRT_ERR_UNSUPPORTED, "prt_set_smooth_normals: more than PRT_MAX_TRIANGLE_SLOTS triangles (corners are addressed by 32-bit indices)");
    std::vector<uint32_t> group_first, member_face;
    bool ids_ok = false;
    try { ids_ok = normals_group_table(corner_group, T, n_groups, group_first, member_face); }
    catch (const std::bad_alloc&) { return fail(c, PRT_ERR_UNSUPPORTED, "prt_set_smooth_normals: no host memory for a table of n_groups + 1 entries (the topology in force stays)"); }
    if (!ids_ok) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_smooth_normals: a group id >= n_groups (the topology in force stays)");
    // everything a generation will ever need, into buffers of their own: a failure here leaves the topology in force as it was
    const size_t corners = 3 * (size_t)T;
    void* nb[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};       // group, first, member, face_f, face_r, nrm
    const size_t bytes[6] = {corners * 4, group_first.size() * 4, corners * 4, (size_t)T * 16, weighting == PRT_NORMALS_AREA ? (size_t)T * 16 : 0, corners * 16};
    const void* src[6] = {corner_group, group_first.data(), member_face.data(), nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 6 && e == hipSuccess; ++k) {
        if (!bytes[k]) continue;
        e = hipMalloc(&nb[k], bytes[k]);
        if (e == hipSuccess && src[k]) e = hipMemcpy(nb[k], src[k], bytes[k], hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        for (void*& p : nb) free_dev(p);
        c->err = std::string("prt_set_smooth_normals: ") + hipGetErrorString(e);
        return PRT_ERR_HIP;
    }
    free_smooth(c);
    c->d_sm_group = nb[0]; c->d_sm_first = nb[1]; c->d_sm_member = nb[2]; c->d_sm_face_f = nb[3]; c->d_sm_face_r = nb[4]; c->d_sm_nrm = nb[5];
    c->smooth_weighting = weighting; c->smooth_crease = crease_cos;
    c->smooth = true;
    return PRT_OK;
}

extern "C" int prt_read_normals(prt_ctx* c, float* normals) {
    CTX_CHECK(c);
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, "prt_read_normals: no scene uploaded");
    if (!normals) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_normals: null pointer");
    const size_t T = c->n_tris;
    if (!T) return PRT_OK;
    std::memset(normals, 0, 3 * T * 4 * sizeof(float));
    if (!c->n_slots) return PRT_OK;
    int rc = prt_synchronize(c);
    if (rc) return rc;
    // the slot table: the uploaded tree's on the host, a rebuilt tree's on the device only
    std::vector<uint32_t> sv;
    if (c->rebuilt) {
        sv.resize(c->n_slots);
        HIPCHK(c, hipMemcpy(sv.data(), c->d_slot_vtx, sv.size() * 4, hipMemcpyDeviceToHost));
    }
    const std::vector<uint32_t>& slot_vtx = c->rebuilt ? sv : c->slot_vtx;
    std::vector<TriNrm> tn(c->n_slots);
    HIPCHK(c, hipMemcpy(tn.data(), c->d_tri_nrm, tn.size() * sizeof(TriNrm), hipMemcpyDeviceToHost));
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
