/*
 * prt.h -- C ABI of libprt: the MI355X-native drop-in for the OpenCL enqueue sequence of the
 * reference renderer (Mourtz/Photorealistic-Rendering-using-OpenCL, src/main.cpp).
 *
 * The reference has no plugin interface for its radiance loop; the boundary is the sequence of
 * OpenCL host calls in src/main.cpp.  Each entry point below replaces one group of those calls
 * (file:line given per function) with the same ownership rule the reference uses
 * (CL_MEM_COPY_HOST_PTR, include/CL/cl_help.h:196-202): the caller keeps ownership of every host
 * array, the library copies on upload.  Plain pointers and sizes only; no C++/torch types.
 *
 * Threading: one context per device; calls on one context are not re-entrant (the reference is
 * single-threaded with an in-order queue and a finish() after every enqueue).  Contexts on
 * different devices may be driven from different threads/processes.
 *
 * Errors: every function returns PRT_OK (0) or a negative prt_status; prt_last_error() gives a
 * message.  The library never aborts or exits (the reference prints and exit(1)s,
 * include/CL/cl_kernel.h:22-28).  There is NO CPU fallback: without a HIP device prt_create fails.
 */
#ifndef PRT_H
#define PRT_H

#include <stdint.h>
#include "prt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRT_ABI_VERSION 3
#define PRT_MAX_LIGHTS 16

typedef enum prt_status {
    PRT_OK = 0,
    PRT_ERR_INVALID_ARGUMENT = -1,
    PRT_ERR_NO_DEVICE = -2,
    PRT_ERR_HIP = -3,
    PRT_ERR_NOT_READY = -4,     /* scene / camera / size not set before rendering */
    PRT_ERR_UNSUPPORTED = -5    /* box primitives: they never render in the reference either (box.cl is not included) */
} prt_status;

/* phase function of the global medium.  The reference wires Isotropic at source level
 * (kernels/media.cl:61); HG (g fixed 0.6, kernels/phasefunctions/HenyeyGreenstein.cl:4) and
 * Rayleigh (kernels/phasefunctions/Rayleigh.cl) exist as files.  Here it is a run-time choice. */
typedef enum prt_phase { PRT_PHASE_ISOTROPIC = 0, PRT_PHASE_HG = 1, PRT_PHASE_RAYLEIGH = 2 } prt_phase;

/*
 * The scene-specialisation parameters of the reference's kernel builder
 * (include/CL/cl_kernel.h:13-446 substitutes them into kernels/header.cl:39-122 as #defines).
 */
#define PRT_VIEW_RESULTS 0u
#define PRT_VIEW_NORMAL 1u
#define PRT_VIEW_BVH_HIT 16u

typedef struct prt_config {
    uint32_t abi_version;            /* PRT_ABI_VERSION */
    int32_t max_bounces;             /* cl_kernel.h:115-122   MAX_BOUNCES            (default 12) */
    int32_t max_diff_bounces;        /* :124-131              MAX_DIFF_BOUNCES       (4)  */
    int32_t max_spec_bounces;        /* :133-140              MAX_SPEC_BOUNCES       (4)  */
    int32_t max_trans_bounces;       /* :142-149              MAX_TRANS_BOUNCES      (12) */
    int32_t max_scattering_events;   /* :151-158              MAX_SCATTERING_EVENTS  (12) */
    int32_t marching_steps;          /* :160-167  MARCHING_STEPS of the raymarched SDF primitives (128) */
    int32_t shadow_marching_steps;   /* :169-176  SHADOW_MARCHING_STEPS (64) */
    uint32_t active_mats;            /* :226-345  ACTIVE_MATS: OR of all material type bits in the scene */
    uint32_t geom_flags;             /* :180-222  PRT_GEOM_* bits for H_SPHERE/H_BOX/H_SDF/H_QUAD */
    uint32_t light_count;            /* :367-400  LIGHT_COUNT */
    uint32_t light_indices[PRT_MAX_LIGHTS]; /*   LIGHT_INDICES (only [0] is ever sampled, base.cl:92 -- unless pick_random_light) */
    int32_t has_global_medium;       /* :47-54    GLOBAL_MEDIUM */
    float fog_density;               /* :66-75    values AFTER the "%f" round trip of std::to_string */
    float fog_sigma_a;               /* :77-84 */
    float fog_sigma_s;               /* :86-93 */
    float fog_sigma_t;               /* :95-102 */
    int32_t fog_abs_only;            /* :104-111 */
    int32_t alpha_testing;           /* :56-63    -alpha */
    int32_t phase_function;          /* prt_phase */
    float phase_g;                   /* HG asymmetry; the reference fixes 0.6 */
    uint32_t view_option;            /* kernels/main.cl:6-15 VIEW_OPTION: PRT_VIEW_RESULTS (0), or PRT_VIEW_NORMAL / PRT_VIEW_BVH_HIT:
                                      * every frame overwrites the accumulator with (ray.normal after radiance(), 1) and the image is the
                                      * accumulator itself (main.cl:143-145,150-152,161).  The other values of the reference's list are
                                      * refused: VIEW_STACK_INDEX does not compile there (Ray has no bvh_stackIndex), VIEW_ALBEDO and
                                      * VIEW_SPECULAR have no branch at all -- radiance() is never called and the image stays black */
    uint32_t pick_random_light;      /* kernels/integrators/base.cl:9 PICK_RANDOM_LIGHT (a source-level `#define ... 0` in the reference): 1 = the
                                      * light of lightSample / volumeLightSample is LIGHT_INDICES[(int)(next1D() * (LIGHT_COUNT + 1))]
                                      * (base.cl:88-90,202-204) -- one draw more per light sample, and an index one PAST the array with
                                      * probability 1 / (LIGHT_COUNT + 1).  That entry is defined here as 0 (mesh 0 is sampled as if it were
                                      * a light), which is what the reference build of the fixtures reads there (the array is declared one
                                      * element longer in the temporary text: zero-initialised).  Needs light_count < PRT_MAX_LIGHTS. */
    uint32_t env_importance_sampling;/* NOT in the reference (it only looks the map up where a ray escapes, pathtracing.cl:72): 1 = at every
                                      * vertex that samples the light (handleSurface, base.cl:168-172) the light-sample strategy is a coin flip
                                      * between LIGHT_INDICES[0] and the ENVIRONMENT MAP, sampled in proportion to its luminance x sin(theta)
                                      * and combined with the BSDF sample by the power heuristic; a BSDF-sampled ray that escapes adds the map
                                      * with the complementary weight and ends its path in that segment.  The expectation of every complete
                                      * path is the one of the default mode, bounce caps included: a vertex whose counters reset the path
                                      * (MAX_BOUNCES, MAX_DIFF_BOUNCES, ...) gets no light from the map in the default mode -- its escaped ray
                                      * would be looked up in a segment that never runs -- and gets none here; the escaped ray's term passes
                                      * the same Russian roulette.  (Limit: a material whose lobes count against DIFFERENT caps -- coat, rough
                                      * dielectric -- at a vertex where only one of them is full takes the map sample or not by the lobe its
                                      * BSDF sample drew; the expectation there is the default's only approximately.)  tests/test_env_sampling.py
                                      * compares 8 x 8 block means of the two modes; the random
                                      * number sequence is not the default's, so this mode has no bit-exact counterpart.  Surfaces only: refused together
                                      * with a global medium, SDF primitives, a debug view or pick_random_light. */
} prt_config;

/* Host buffers of one scene, in the reference's layouts (src/main.cpp:93-122,401-418). */
typedef struct prt_scene_desc {
    const prt_mesh* meshes;          /* cl_meshes  src/main.cpp:418: order spheres, sdfs, boxes, quads */
    uint32_t object_count[8];        /* kernel arg 3 (cl_uint8): n_sphere,n_sdf,n_box,n_quad,_,_,_,total  include/Scene/scene.h:20-22 */
    const prt_material* obj_material;/* mBufMaterial src/main.cpp:403-404: ONE material for the whole OBJ (may be NULL if no OBJ) */
    const float* vertices;           /* mBufVertices :117  float4[3*T], de-indexed, xyz used */
    const float* normals;            /* mBufNormals  :118  float4[3*T] */
    const uint64_t* primitive_indices;/* mNewBufIndices :119 cl_ulong[T] */
    uint32_t triangle_count;         /* T */
    const prt_bvh_node* bvh_nodes;   /* mNewBufBVH :412   node 0 = root */
    uint32_t bvh_node_count;
} prt_scene_desc;

typedef struct prt_stats {
    double kernel_ms;        /* device time of the render kernels of the last prt_render_* call (HIP events on the context's
                                stream, around everything the call queued: wall time of the GPU work) */
    uint32_t launches;       /* kernel launches in that call */
    uint32_t frames;         /* frames (= segments per live pixel) executed in that call */
    uint64_t samples;        /* sum over pixels of RLH.samples (paths started)   -- filled by prt_query_counts */
    uint64_t segments;       /* sum over pixels of acc.w (segments executed)     -- filled by prt_query_counts */
    uint64_t finished_pixels;/* pixels frozen by the spp rule                     -- filled by prt_query_counts */
    double kernel_sum_ms;    /* sum of the durations of the individual launches (HIP events around each launch on the
                                stream it ran on; prt_render_spp only, else = kernel_ms).  The megakernel keeps
                                `concurrent` launches in flight (interleaved sets of tiles on internal streams), so
                                kernel_sum_ms ~ concurrent x kernel_ms; kernel_sum_ms / launches is what a profiler
                                reports as the kernel's average duration */
    uint32_t concurrent;     /* launches in flight at a time (internal streams; PRT_STREAMS, default 2) */
    uint32_t _pad;
} prt_stats;

typedef struct prt_ctx prt_ctx;

/* initOpenCL(), src/main.cpp:124-209 + cl_help::kernel::parse: pick the device and specialise
 * the integrator for one scene.  `device` is a HIP device ordinal. */
int prt_create(int device, const prt_config* cfg, prt_ctx** out);

/* process exit in the reference; explicit here. */
void prt_destroy(prt_ctx* ctx);

/* Size limits of the device tables.  The render kernels address the node pairs (64 bytes each), the triangle records of the leaf slots
 * (48 bytes each, one slot per leaf reference of a triangle) and the materials (48 bytes each, object_count[7] + 2 records) by a 32-bit byte
 * offset from the table's base: each table stays below 4 GiB.  A scene, a refit or a device rebuild whose tables would be larger is refused
 * with PRT_ERR_UNSUPPORTED and a message that names the limit it passed. */
#define PRT_MAX_TRIANGLE_SLOTS 89478485u   /* floor((2^32 - 1) / 48) */
#define PRT_MAX_NODE_PAIRS 67108863u       /* 2^26 - 1 */
#define PRT_MAX_MATERIALS 89478485u        /* floor((2^32 - 1) / 48); the 24-bit mesh index of a hit record binds first */
#define PRT_MAX_ENV_TEXELS 357913941u      /* floor((2^32 - 1) / 12): prt_upload_envmap, width x height of the RGB float map */
#define PRT_MAX_ENV_SIDE 16777215          /* 2^24 - 1: prt_upload_envmap, width and height each (the texel index is a 24-bit multiply) */

/* clw::buffer::create x5 + mBufMaterial, src/main.cpp:401-418,93-122.  Copies and re-packs.  PRT_ERR_UNSUPPORTED beyond the limits above. */
int prt_upload_scene(prt_ctx* ctx, const prt_scene_desc* scene);

/* Deforming geometry: new vertices into the uploaded scene, the tree REFITTED on the device (no counterpart in the reference, whose scene is
 * static: moving a triangle there means rebuilding the tree and creating every buffer again, as prt_upload_scene does here).  The tree's
 * topology is kept -- which node is whose child, which triangles a leaf holds --; the triangle records and every box are recomputed from the
 * new vertices, bottom-up.  T, primitive_indices and bvh_nodes are those of the last prt_upload_scene; `vertices` and `normals` have the layout
 * of prt_scene_desc: float4[3*T], de-indexed, xyz used.  normals == NULL keeps the uploaded normals (they are not read) -- or,
 * with prt_set_smooth_normals (below), generates them from the new vertices.
 *   prt_update_vertices          host memory: staged through a device buffer of the context (allocated on first use), then the device path.
 *   prt_update_vertices_device   device memory of the context's device, 16-byte aligned; ordered on the context's stream, complete on return
 *                                (the caller's buffers may be reused then).
 * All operations f32, no contraction.  A "slot" is one triangle reference of a leaf: the leaves' triangles in the order the library stores
 * them, slot_src[s] = the position in primitive_indices that slot s came from (a leaf's slots are consecutive and in the leaf's order).
 *   Triangle record of slot s: fv = (uint32)primitive_indices[slot_src[s]] * 3 (kernels/geometry/triangle.cl:7);  p0 = v[fv],
 *     e1 = p0 - v[fv+1], e2 = v[fv+2] - p0 (triangle.cl:12-13), n = cross(e1, e2) with the component expressions of triangle.cl:15:
 *     n.x = e1.y*e2.z - e1.z*e2.y, n.y = e1.z*e2.x - e1.x*e2.z, n.z = e1.x*e2.y - e1.y*e2.x.  With normals: the three normals of fv, fv+1, fv+2
 *     copied, lane 3 = 0.  These are prt_upload_scene's own expressions: the records equal those of an upload of the new vertices.
 *   Leaf box: per axis lo = hi = the coordinate of vertex 0 of the leaf's first slot; every further vertex follows in slot order, vertices
 *     0, 1, 2 of each slot:  lo = c < lo ? c : lo;  hi = c > hi ? c : hi  (std::min(lo, c) / std::max(hi, c) as the host builder calls them,
 *     csrc/host/bvh.cpp).  The comparison form is part of the contract: it fixes the sign of a zero bound (of +0.0 and -0.0 the one that came
 *     first stays).  A leaf with primitive_count == 0 keeps the box it was uploaded with.
 *   Inner box: the box of child 0 of the node (first_child_or_primitive), then child 1's box merged per axis by the same two comparisons
 *     (c = child 1's lo for lo, its hi for hi).  Children before parents.
 *   Root box: the same union over the root's two children, or the leaf rule when the root is a leaf.
 *   A caller's tree with loose boxes comes out tight.
 * The result is deterministic: tile, row-block and multi-rank contexts each call it on their own context and the union of their renders
 * stays bit-identical to one whole-frame context's; a render after an update equals a render after prt_upload_scene of the same vertices,
 * normals and the refitted nodes, bit for bit.
 * Lifetime: an update makes the guides stale and forgets measured tile orders, as prt_set_camera does.  It keeps the path state, the
 * framebuffer (unchanged until the next render) and both temporal histories.  The loop per displayed frame: update, prt_reset, render,
 * prt_render_guides, prt_denoise_temporal.  Without motion (prt_set_motion, below: off by default) the reprojection treats every surface as if it
 * had stood still: its depth and normal tests reject most surfaces that moved (their history restarts), and where they happen to pass the
 * history of another surface point is blended in.  With motion on, the guide render also says where each pixel's point of the mesh was
 * before the update and the reprojection looks there: the history follows the deforming mesh (and, through prt_update_primitives below, a
 * moving sphere, quad or SDF primitive).  What still does not follow: surfaces seen through mirrors or glass (the virtual point behind a
 * delta chain carries no motion), and a surface that turns by more than cos_n between two frames (the normal test compares the current normal
 * with the one stored in the previous frame; previous-frame normals are out of scope) -- those restart.  prt_reset_history empties it.  Spheres,
 * quads, SDF primitives and materials are not touched: prt_update_primitives (below) moves the former three.  The tables a refit needs (4 bytes per slot
 * and per inner node) go to the device with the first update: a static scene costs no device memory.
 * Refused, each leaving the scene exactly as it was: PRT_ERR_NOT_READY without a scene or with T == 0; PRT_ERR_INVALID_ARGUMENT for null
 * `vertices`, a misaligned device pointer, or any non-finite x, y or z among the 3T vertices (the loaders refuse those too: a NaN box hides
 * its subtree); PRT_ERR_UNSUPPORTED for a tree whose inner nodes are nested more than 256 deep (the boxes take one launch per level; the
 * traversal-stack bound of prt_upload_scene counts only nodes with two inner children, so a caller's chain can be deeper: such a tree still
 * uploads and renders).
 * prt_read_bvh_bounds: 6 floats per node of the uploaded tree, in ITS node numbering: min_x max_x min_y max_y min_z max_z (the layout of
 * prt_bvh_node::bounds).  Before any update the uploaded bounds, after one the refitted ones; the root (stored nowhere on the device before
 * an update) by the rule above, a leaf root before any update as uploaded.  A node that no inner node names as a child reads as six zeros.
 * PRT_ERR_NOT_READY without a scene. */
int prt_update_vertices(prt_ctx* ctx, const float* vertices, const float* normals);
int prt_update_vertices_device(prt_ctx* ctx, const void* d_vertices, const void* d_normals);
int prt_read_bvh_bounds(prt_ctx* ctx, float* bounds6);

/* Moving spheres, quads and SDF primitives: new prt_mesh records into the uploaded scene, in place (no counterpart in the reference).  `count`
 * must equal object_count[7] of the last prt_upload_scene; record i is mesh i of that upload: spheres first, then SDF primitives, then quads.
 *   prt_update_primitives          host memory: staged through a device buffer of the context (allocated on first use), then the device path.
 *   prt_update_primitives_device   device memory of the context's device, 16-byte aligned, count x 256 bytes; ordered on the context's stream,
 *                                  complete on return (the caller's buffer may be reused then).
 * Only geometry is read -- sphere: pos[0..2], joker[0] (radius); SDF primitive: pos[0..2], joker[0..3]; quad: joker[0..12] (base, edge0, edge1,
 * normal, area, as the caller gives them) -- and t, which must equal the uploaded record's: kind and SDF sub-type are fixed.  mat, the
 * paddings and the other joker entries are not read; the materials table is not touched.  The resulting sphere, SDF and quad tables are, byte
 * for byte, what prt_upload_scene of the same scene with these meshes makes (the quad's anchor = base - (edge0 + edge1) * 0.5f, dot(edge0,
 * edge0), dot(edge1, edge1) and their half-ulp bounds included): a render after the call is bit-identical to a fresh context that uploads the
 * moved scene; tile, row-block and rank contexts that each call it stay bit-identical in union to one whole-frame context.
 * Lifetime: that of prt_update_vertices.  The guides go stale and measured tile orders are forgotten; the path state, the framebuffer, both
 * temporal histories, the refit and rebuild tables, the smoothing topology and a pending triangle snapshot are kept.  The loop per displayed
 * frame: update, prt_reset, render, prt_render_guides, prt_denoise_temporal.  A scene without triangles, or without one or two of the three
 * kinds, is accepted.  The staging tables (and, with motion on, the previous tables) are allocated by the first call: a scene that never
 * moves a primitive pays nothing.
 * Refused, each leaving the scene and a pending snapshot exactly as they were: PRT_ERR_NOT_READY without a scene; PRT_ERR_INVALID_ARGUMENT for
 * a wrong count, a null pointer, a misaligned device pointer, a record whose t differs from the uploaded one, or a non-finite value in a field
 * that is read (a non-finite value in a field that is not read is not looked at).  The records are packed and checked on the device into
 * staging tables; the host reads the check's flag before anything live is overwritten.  count == 0 on a scene without primitives succeeds and
 * does nothing.
 * With prt_set_motion on, an accepted update keeps the three tables as they were (see "Snapshot" under prt_set_motion). */
int prt_update_primitives(prt_ctx* ctx, const prt_mesh* meshes, uint32_t count);
int prt_update_primitives_device(prt_ctx* ctx, const void* d_meshes, uint32_t count);

/* Deforming geometry, second door: new vertices into the uploaded scene and a NEW TREE over all T triangles, built on the device in Morton order
 * (no counterpart in the reference).  Arguments, alignment and staging are those of prt_update_vertices / prt_update_vertices_device; the call
 * is ordered on the context's stream and complete on return.  max_leaf = 1 .. 64, 0 = the library's default (4).  Triangle i is vertices 3i,
 * 3i+1, 3i+2; what the tree being replaced looked like does not matter (one that referenced 100 of T triangles comes back with T), so a mesh
 * may be uploaded under a trivial tree -- a leaf root that names every triangle -- and get its real one here.
 * The tree, all f32, no contraction:
 *   1. Triangle box: the leaf rule of prt_update_vertices over the triangle's three vertices.  Centre per axis: c = lo * 0.5f + hi * 0.5f.
 *   2. Extent of the centres per axis: lo = (min over all triangles) + 0.0f, hi = (max over all triangles) + 0.0f (the sign of a zero cannot
 *      depend on the order of the reduction); scale = hi > lo ? 1024.0f / (hi - lo) : 0.0f.
 *   3. q = (uint32) min((c - lo) * scale, 1023.0f) per axis (min(t, 1023) = t < 1023.0f ? t : 1023.0f); the 30-bit Morton code interleaves
 *      the 10 bits of q.x, q.y, q.z with x in the highest bit of each triple, then y, then z.
 *   4. key = (uint64)code << 32 | i: distinct, sorted ascending.
 *   5. The binary radix tree of the sorted keys: a range [a, b] of positions with a < b splits behind the largest g in [a, b) whose key has a 0
 *      in the highest bit in which key[a] and key[b] differ, into [a, g] and [g + 1, b].  A range of at most max_leaf triangles is a leaf;
 *      T <= max_leaf gives a leaf root.
 *   6. The inner ranges ("pairs") are numbered by (depth, first position): breadth-first, left to right, the root pair 0.  Node 0 is the
 *      root; the children of pair k are nodes 2k + 1 and 2k + 2.
 *   7. Slots: the leaves in pair order, a pair's left leaf first; within a leaf the triangles in sorted order.  primitive_indices[s] is the
 *      triangle of slot s, a leaf's first_child_or_primitive its first slot (prt_upload_scene's own slot order).
 *   8. Boxes and triangle records: the rules of prt_update_vertices on the new tables.
 *   9. Every device buffer and table equals what prt_upload_scene of (new vertices, new normals, the tree of 1 - 8) makes with breadth-first
 *      pair order.  The key has 62 significant bits: depth <= 62, within the 64-entry traversal stack and the 256 levels of a refit.
 * A render after a rebuild is bit-identical to a fresh context that uploads what prt_read_bvh returns; prt_update_vertices afterwards refits
 * the new topology; tile, row-block and rank contexts that each rebuild stay bit-identical in union to one whole-frame context.
 * Lifetime: as an update -- path state, framebuffer and both histories are kept, guides and measured tile orders dropped.  normals == NULL
 * carries the normal records to the new slots (through "a slot of the old tree that holds the triangle": where leaves shared a triangle
 * their records are equal).  With prt_set_motion on, the snapshot the motion plane is measured from moves to the new slot order the same
 * way: a pending one is permuted, otherwise the current records are taken; a triangle the old tree did not hold gets its new record (no
 * motion).  The history follows the mesh across a rebuild as across an update.
 * Refused, each leaving the scene exactly as it was (the tree is built into buffers of its own and swapped in at the end): what
 * prt_update_vertices refuses (the 256-level limit apart: the old tree is not refitted), max_leaf > 64, and normals == NULL when the current
 * tree does not reference every triangle (there is no normal record for the rest): PRT_ERR_INVALID_ARGUMENT.  T - 1 > PRT_MAX_NODE_PAIRS (the
 * pair table is sized for a tree of single-triangle leaves): PRT_ERR_UNSUPPORTED.
 * prt_read_bvh: the current tree in the reference's layout, node 0 the root: an uploaded tree as uploaded with its current boxes, a
 * rebuilt one by rules 6 and 7 (inner nodes: primitive_count 0).  nodes == NULL writes *node_count only; primitive_indices (may be NULL)
 * receives T entries.  prt_read_bvh_bounds keeps working, in the numbering prt_read_bvh returns. */
int prt_rebuild_bvh(prt_ctx* ctx, const float* vertices, const float* normals, uint32_t max_leaf);
int prt_rebuild_bvh_device(prt_ctx* ctx, const void* d_vertices, const void* d_normals, uint32_t max_leaf);
int prt_read_bvh(prt_ctx* ctx, prt_bvh_node* nodes, uint32_t* node_count, uint64_t* primitive_indices);

/* Deforming geometry: smooth shading normals regenerated on the device (no counterpart in the reference, whose normals come from the importer
 * once: GenSmoothNormals of assimp, csrc/host/model_loader.cpp smooth_missing_normals here).  Opt-in; off (the default) every bit of every
 * result is what it is without these calls: normals == NULL keeps / carries the normal records, which after a deformation are the rest
 * pose's.  The caller gives the mesh's smoothing topology once; from then on every prt_update_vertices, prt_update_vertices_device,
 * prt_rebuild_bvh and prt_rebuild_bvh_device called with normals == NULL generates the float4[3T] normals from the new vertices -- after the
 * finite-vertex check has passed, into a buffer of the context, so a refused call still leaves the scene exactly as it was -- and proceeds
 * exactly as if that array had been passed as `normals` (prt_rebuild_bvh's refusal of normals == NULL under a tree that does not reference
 * every triangle does not apply then: there is a normal for every corner).  Explicit normals are used as without the topology;
 * prt_set_motion reads geometry records only and is unaffected.
 * Corner c = 3i + k is vertex k of triangle i of prt_scene_desc::vertices.  The topology is a group id per corner: the corners of one group
 * share their faces' normals.  All f32, no contraction; sqrtf and / correctly rounded:
 *   Face i, with a = v[3i], b = v[3i+1], c = v[3i+2] (xyz):
 *       u = b - a;   w = c - a
 *       r = (u.y*w.z - u.z*w.y,  u.z*w.x - u.x*w.z,  u.x*w.y - u.y*w.x)
 *       l = sqrtf((r.x*r.x + r.y*r.y) + r.z*r.z);     f = l > 0 ? r / l (per component) : r
 *     (unit_face_normal of the loader.  It points the opposite way from the triangle record's n = cross(e1, e2), kernels/geometry/triangle.cl:15,
 *     and is not derived from that record: the signs of zeros would differ.)
 *   Corner c of face i, in group g with members m_0 < m_1 < ... (corner indices, c itself among them; face j = m / 3):
 *       s = 0
 *       for each member in that order:
 *           d = (f_j.x*f_i.x + f_j.y*f_i.y) + f_j.z*f_i.z
 *           if (d >= crease_cos)  s += (PRT_NORMALS_UNIT ? f_j : r_j)    per component
 *       L = sqrtf((s.x*s.x + s.y*s.y) + s.z*s.z);     normal = L > 0 ? s / L : f_i;     lane 3 = 0
 *     A face counts once per corner it has in the group.  NaN and overflow go through the formulas as they stand; a NaN d fails the test.
 *   With PRT_NORMALS_UNIT, PRT_LOADER_CREASE_COS and the groups of prt_weld_corners this is smooth_missing_normals operation for operation, for
 *   a single-mesh model.
 * Deterministic, no atomics: the result depends on the vertices and the topology only; tile, row-block and rank contexts that each set the
 * same topology and update stay bit-identical in union to one whole-frame context.
 * Cost: two launches in front of the refit's record pass -- one lane per triangle, then one lane per corner that gathers one 16-byte face
 * record per member of its group: the sum over the groups of valence^2 gathers.  A pole of valence 1000 is slow but correct.
 * Device memory, all allocated by prt_set_smooth_normals (an update cannot fail on an allocation after the scene has been touched), per
 * triangle: 12 bytes of ids, 12 of the member table, 16 of face records {f, l} (PRT_NORMALS_AREA: 16 more, {r, 0}) and 48 of generated
 * normals -- 88 (104) bytes -- plus 4 * (n_groups + 1) bytes of group offsets.
 * prt_weld_corners (host only: no device, no context, as prt_env_cdf): corners whose positions are bit-identical after x + 0.0f per component
 *   (so -0 equals +0: the key of smooth_missing_normals) form one group; groups are numbered in order of first appearance by corner index.
 *   PRT_ERR_INVALID_ARGUMENT (message: prt_last_global_error) for null pointers, T == 0 or a non-finite x, y or z.  Callers who want hard
 *   edges or seams pass ids of their own to prt_set_smooth_normals.
 * prt_set_smooth_normals: copies the ids, builds the group-to-members table on the host (a stable counting sort: a group's members in
 *   ascending corner order; an id no corner names is an empty group) and uploads it.  Needs an uploaded scene with T > 0, else
 *   PRT_ERR_NOT_READY.  Refused with PRT_ERR_INVALID_ARGUMENT, each leaving the previous topology in force: an id >= n_groups, n_groups == 0,
 *   an unknown weighting, a crease_cos that is not finite.  PRT_ERR_UNSUPPORTED for T > PRT_MAX_TRIANGLE_SLOTS (corners are 32-bit indices).
 *   corner_group == NULL turns the feature off and frees the buffers.  Setting it changes nothing of the scene by itself: records, guides and
 *   histories keep their bits until the next update or rebuild.  It survives prt_reset, prt_resize, tile and row-block calls, camera changes,
 *   updates and rebuilds; prt_upload_scene turns it off (T may have changed).
 * prt_read_normals: the current normal records de-slotted into corner order, float4[3T]: for triangle i the three normals of a slot that
 *   holds it (where leaves share a triangle their records are equal), lane 3 = 0; a triangle that no slot holds reads as zeros.  For an
 *   uploaded, a refitted and a rebuilt tree, smooth normals on or off.  PRT_ERR_NOT_READY without a scene, PRT_ERR_INVALID_ARGUMENT for a
 *   null pointer. */
#define PRT_NORMALS_UNIT 0u   /* sum of the faces' unit normals: the loader's / assimp's rule */
#define PRT_NORMALS_AREA 1u   /* sum of the faces' raw cross products: area-weighted */
#define PRT_LOADER_CREASE_COS (-0.99619470f)   /* cos(175 deg): the smoothing-angle limit of the loader */
int prt_weld_corners(const float* vertices /* float4[3T] */, uint32_t T, uint32_t* corner_group /* 3T */, uint32_t* n_groups);
int prt_set_smooth_normals(prt_ctx* ctx, const uint32_t* corner_group /* 3T, NULL = off */, uint32_t n_groups, uint32_t weighting, float crease_cos);
int prt_read_normals(prt_ctx* ctx, float* normals /* float4[3T] */);

/* enqueueWriteBuffer(cl_camera), src/main.cpp:294-297 (every frame in the reference). */
int prt_set_camera(prt_ctx* ctx, const prt_camera* cam);

/* cl_env_map, src/main.cpp:433-437 + include/GL/cl_gl_interop.h:71-86: RGB float, row 0 first.
 * Without a call the map is a 1x1 black texel.  The map is the context's, not the scene's: it survives prt_upload_scene. */
int prt_upload_envmap(prt_ctx* ctx, const float* rgb, int width, int height);

/* cl_flattenI = W*H*112 bytes, src/main.cpp:451; output texture tex0.  Implies prt_reset. */
int prt_resize(prt_ctx* ctx, int width, int height);

/* Multi-GPU row tile: this context renders rows [row0, row0+rows) of the width x full_height
 * image; seeds and camera use GLOBAL pixel coordinates so the union of tiles is bit-identical to
 * a single-context render.  State/framebuffer calls then address the tile only.  Implies reset. */
int prt_set_tile(prt_ctx* ctx, int width, int full_height, int row0, int rows);

/* Interleaved variant for load balance: the frame is cut into blocks of `block_rows` rows and
 * this context owns blocks part, part + n_parts, part + 2 n_parts, ... (local row order = global
 * row order of the owned rows).  State/framebuffer calls address the owned rows only. */
int prt_set_row_blocks(prt_ctx* ctx, int width, int full_height, int block_rows, int n_parts, int part);

/* buffer_reset branch of render(), src/main.cpp:283-291: zero the path state. */
int prt_reset(prt_ctx* ctx);

/* setArg(4,++framenumber); setArg(6,rand()); setArg(7,rand()); enqueueNDRangeKernel; finish --
 * src/main.cpp:299-304,260-261 -- batched: frames first_frame .. first_frame+n-1 (frame numbers
 * start at 1), seed_pairs = {random0, random1} per frame.  Every pixel advances one path segment
 * per frame.  Asynchronous on the context's stream; prt_synchronize / any read waits. */
int prt_render_frames(prt_ctx* ctx, uint32_t first_frame, uint32_t n_frames, const int32_t* seed_pairs);

/* "N spp": frames 1,2,... with a pixel frozen once its N-th path has terminated
 * (reset && samples == spp).  Runs until every pixel is frozen or max_frames frames were used;
 * seed_pairs must hold max_frames pairs.  *frames_used (optional) receives the frames launched: the frame count
 * of the slowest pixel rounded up to the launch size, at most max_frames.  A pixel's result depends on its own frames
 * only, so the launches let a pixel whose wave waits for slower neighbours start on the frames of the next launch
 * (the per-pixel lead lives in the device state for the duration of the call; PRT_RUN_AHEAD=0 turns it off); if
 * max_frames is reached (PRT_ERR_NOT_READY) every unfrozen pixel has done exactly max_frames.
 * Requires a freshly reset context. */
int prt_render_spp(prt_ctx* ctx, uint32_t spp, uint32_t max_frames, const int32_t* seed_pairs,
                   uint32_t* frames_used);

/* Adaptive sampling (no counterpart in the reference): "N spp" with a per-pixel N.  Frames 1, 2, ... as prt_render_spp (same
 * preconditions: a freshly reset context -- PRT_ERR_NOT_READY otherwise --, seed_pairs for max_frames frames, PRT_ERR_NOT_READY when max_frames
 * runs out with pixels unfrozen, each of them then having done exactly max_frames frames), under this freeze rule:
 *
 *   Per pixel a plane {l, s2} (8 bytes, allocated on first use, zeroed by prt_reset / prt_resize / prt_set_tile / prt_set_row_blocks) is
 *   updated at the end of every path (a segment that leaves reset set), after the accumulate of acc (kernels/main.cl:142).  f32 operations,
 *   left to right, no contraction:
 *       lum = 0.2126f*acc.x + 0.7152f*acc.y + 0.0722f*acc.z;   y = lum - l;   s2 = s2 + y*y;   l = lum
 *   At that path end, with n = samples >= min_spp, the pixel is judged (IEEE division):
 *       m = l / n;   v = fmaxf((s2 - l*m) / ((float)n * (float)(n - 1)), 0);   t = rel_err * fmaxf(m, abs_floor);   converged = v < t*t
 *   (v is clamped because the difference can round below zero when every path brought the same luminance; strict: rel_err = 0 never
 *   converges).  The pixel freezes when reset && (samples >= max_spp || converged).  The converged bit lives in
 *   the device state between launches (bit 31 of the state word that also holds reset); prt_read_state and the RTD layout do not show it --
 *   a frozen pixel with samples < max_spp was frozen by convergence.
 *
 * A pixel frozen after k paths is bit-identical (path state and framebuffer) to the same pixel of prt_render_spp(k).  Refused: min_spp < 2,
 * max_spp < min_spp, rel_err or abs_floor negative or NaN (PRT_ERR_INVALID_ARGUMENT); a debug view (PRT_ERR_UNSUPPORTED: it overwrites acc).
 * Once fewer than a fraction of the frame's pixels are live, the launches run over a list of the live pixels packed 64 to a wave (option
 * "compact"); run-ahead and pacing apply as in prt_render_spp, the tile order and the ray pool do not. */
typedef struct prt_adaptive {
    uint32_t min_spp;     /* >= 2 */
    uint32_t max_spp;     /* >= min_spp */
    float rel_err;        /* target relative standard error of the pixel's mean luminance; 0 = never converge (pure max_spp) */
    float abs_floor;      /* mean luminance below which the error is judged absolutely (dark pixels) */
} prt_adaptive;
int prt_render_adaptive(prt_ctx* ctx, const prt_adaptive* a, uint32_t max_frames, const int32_t* seed_pairs, uint32_t* frames_used);
/* the plane {l, s2} per pixel, framebuffer order (2 floats per pixel; zeros before the first adaptive render of a reset context) */
int prt_read_adaptive_stats(prt_ctx* ctx, float* out2);
/* what the last prt_render_adaptive did with its launches */
typedef struct prt_adaptive_report {
    uint32_t tile_launches;      /* launches over tiles (or scattered pixels) */
    uint32_t list_launches;      /* launches over a live-pixel list */
    uint32_t list_builds;        /* lists built */
    uint32_t _pad;
    uint64_t list_lanes;         /* lanes of the list launches' waves (64 per wave) */
    uint64_t list_live_lanes;    /* ... that held a pixel still live when its launch was issued */
} prt_adaptive_report;
int prt_get_adaptive_report(prt_ctx* ctx, prt_adaptive_report* out);

/* Guide (feature) buffers (no counterpart in the reference: its VIEW_ALBEDO is named, kernels/main.cl:6-15, but has no branch).
 * prt_render_guides traces `samples` (1 .. 64) guide samples per pixel of the context's frame part (tiles and row blocks included: global
 * pixel coordinates, as the render kernel):
 *   - Sample s sits at the fractional pixel offset (fx, fy) = (0.5, 0.5) for s = 0, else ((0.5 + s*0.7548776662) mod 1, (0.5 + s*0.5698402910)
 *     mod 1) (the R2 sequence, f32).  The camera ray is create_cam_ray's (kernels/camera.cl:17-66) through the image-plane point
 *     sx = (x + fx - 0.5) / (width - 1), sy = (height - 1 - y - (fy - 0.5)) / (height - 1) -- (fx, fy) = (0.5, 0.5) is the point the render
 *     samples -- and, with apertureRadius > 0.00001, the lens sample (random1, random2) = ((fx + 0.25) mod 1, (fy + 0.75) mod 1).
 *   - Delta chain: at a smooth conductor (PRT_MAT_COND without PRT_MAT_ROUGH_COND) the ray reflects about the shading normal; at a smooth
 *     dielectric (PRT_MAT_DIEL without PRT_MAT_ROUGH_DIEL) it refracts with the index dielectric_sample uses (the material's eta.x, inverted
 *     when the ray arrives on the side the shading normal points to), or reflects on total internal reflection.  At most 4 such events are followed;
 *     the hit after them -- or the first non-delta hit -- gives the sample's values.  Albedo is multiplied by each conductor's
 *     clamp(color, 0, 1) on the way (a dielectric's tint is 1); depth is the summed path length of the chain.
 *   - Per hit: albedo = clamp(material color, 0, 1) (lights included); normal = the shading normal finish_closest yields (interpolated for
 *     triangles), negated when dot(n, dir) > 0.  The global medium, alpha testing and env importance sampling are ignored.
 *   - Miss: albedo = clamp(env lookup of the direction, 0, 1) (times the chain's tint), no hit.
 *   - Per pixel 8 floats, framebuffer order: {albedo.rgb mean over the samples, coverage = hits / samples, normal = normalize(sum over
 *     hits of the finite normals) (0 without hits or for a zero sum), depth = mean over hits (0 without hits)}.
 * The plane is allocated on first use.  It goes stale on prt_upload_scene, prt_set_camera, prt_upload_envmap, prt_resize, prt_set_tile and
 * prt_set_row_blocks (prt_reset keeps it).  prt_read_guides: PRT_ERR_NOT_READY while there are no valid guides. */
int prt_render_guides(prt_ctx* ctx, uint32_t samples);
int prt_read_guides(prt_ctx* ctx, float* out8);

/* Motion of deforming geometry into the temporal reprojection (no counterpart in the reference).  Opt-in: prt_set_motion(ctx, 1); off (the
 * default) every bit of every result is what it is without these calls.
 * The motion plane: per pixel of the context's frame part one more float4 {D.x, D.y, D.z, m}, written by prt_render_guides with motion on.  IT
 * DESCRIBES THE DISPLACEMENT OF THE GEOMETRY BETWEEN THE PREVIOUS prt_render_guides AND THIS ONE:
 *   Snapshot: with motion on, prt_update_vertices / prt_update_vertices_device copy the triangle records (48 bytes per slot; the buffer is
 *     allocated by the first such update) before the refit overwrites them -- after every refusal is decided (a refused update leaves the
 *     snapshot as it was), one device-to-device copy on the context's stream, and only when no snapshot is pending: of several updates
 *     between two guide renders the oldest geometry is kept.  prt_render_guides with motion on measures from the pending snapshot and
 *     consumes it; without one (no update since the last guide render) the plane is all zeros.  The rule is the context's own: a rank that
 *     only renders and exports behaves as the one that filters.  prt_upload_scene and turning motion off drop the snapshot and free it.
 *   Per guide sample s whose FIRST hit (no delta event before it) is a mesh triangle -- the triangle wins finish_closest against spheres,
 *     quads and SDF primitives --, with (slot, u, v) that hit, f32, no contraction, per component:
 *         q(rec) = (rec.p0 - rec.e1 * u) + rec.e2 * v       (p1 = p0 - e1, p2 = p0 + e2; u weighs vertex 1, v vertex 2, as the hit's normal)
 *         d_s    = q(tri_prev[slot]) - q(tri_geom[slot])    (where the point was, minus where it is; exactly 0 for an unchanged record)
 *     Triangle hits contribute only while a triangle snapshot is pending.
 *   Primitive snapshot: with motion on, an accepted prt_update_primitives / prt_update_primitives_device keeps the sphere, SDF and quad tables
 *     as they were -- after every refusal is decided, and only when no primitive snapshot is pending (the oldest wins).  prt_render_guides
 *     consumes it; prt_upload_scene and turning motion off drop it.  It is independent of the triangle snapshot.
 *   Per guide sample s whose FIRST hit is a sphere, a quad or an SDF primitive (mesh index >= 0) of a non-delta material, while a primitive
 *     snapshot is pending, with p the hit position (ray.pos), f32, no contraction, IEEE divides and square root, per component:
 *         sphere i:         w = p - c_cur, h = w / sqrt((w.x w.x + w.y w.y) + w.z w.z);  d_s = (c_prev - c_cur) + h * (r_prev - r_cur)
 *         quad j:           w = p - anchor_cur, a = dot(w, e0_cur) / e0e0_cur, b = dot(w, e1_cur) / e1e1_cur (dot(x, y) = (x.x y.x + x.y y.y) + x.z y.z;
 *                           the quad test measures from anchor, not base);  q(rec) = (rec.anchor + rec.edge0 * a) + rec.edge1 * b;
 *                           d_s = q(prev) - q(cur): translation, rotation and resizing of the card are carried
 *         SDF primitive k:  d_s = pos_prev - pos_cur: only translation is carried, a parameter change carries no motion
 *     Each is exactly +0 for an unchanged record.  Primitive hits contribute only while a primitive snapshot is pending: after
 *     prt_update_vertices alone primitive pixels read as zeros, after prt_update_primitives alone triangle pixels do, after both both carry
 *     motion.  A mirror or glass sphere that moves carries no motion.
 *     Hits behind a mirror or glass chain and misses contribute nothing.
 *   Per pixel: D = (sum of d_s in sample order) / (float)hits (IEEE division; hits = the guides' own hit count: the mean over the hits, as the
 *     guides' depth), m = (float)contributing_samples * (1 / samples).  hits == 0, or no snapshot pending: D = 0, m = 0.
 *   The eight guide floats are the same bits with motion on and off; tiles and row blocks work as for the guides (global coordinates: the
 *     union of the parts is the whole frame's plane bit for bit).
 * In the reprojection (prt_denoise_temporal, below): a covered pixel with m > 0 and (D.x, D.y, D.z) != (0, 0, 0) takes
 *     e = ((position + d * z_p) + D) - P_prev
 *   and everything downstream unchanged: dist = |e|, the projection, the taps' depth test against the previous guides, the normal test (the
 *   current normal against the stored one: a surface that turns by more than cos_n restarts), the blend.  Every other pixel, and a call
 *   without a plane, takes the expressions of prt_denoise_temporal as they stand: a plane of zeros gives the same bits as no plane.
 * prt_set_motion: default 0.  A change makes the guides stale and keeps both histories; a call with the value in force does nothing.  PRT_ERR_UNSUPPORTED with a debug view.  A scene without
 *   triangles is accepted: its planes are zeros unless a primitive moved.
 * prt_read_motion: width * rows * 4 floats, framebuffer order.  PRT_ERR_NOT_READY while motion is off or there are no valid guides rendered
 *   with motion on; PRT_ERR_INVALID_ARGUMENT for a null pointer or a context without a frame size.
 * prt_export_motion: the plane of the frame part (whole frame, tile or row blocks) into device memory of the caller, ordered on the
 *   context's stream as prt_export_denoise_inputs.  Refused as prt_read_motion, and for a pointer that is not 16-byte aligned.  Both calls
 *   write nothing of the context.
 * prt_denoise_temporal uses the context's plane when motion is on and the plane belongs to the valid guides; prt_denoise_records_temporal_motion
 *   (below) takes it as an argument beside the records, whose 64-byte layout is unchanged. */
int prt_set_motion(prt_ctx* ctx, int enable);
int prt_read_motion(prt_ctx* ctx, float* out4);
int prt_export_motion(prt_ctx* ctx, void* device_motion);

/* Denoiser: the spatial part of SVGF (Schied et al. 2017), an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010), guided by the
 * guides above.  L(c) = 0.2126 r + 0.7152 g + 0.0722 b.  Inputs: the framebuffer colour c, the guides {a, cov, n, z} and the luminance
 * variance of the pixel's mean, v, from
 *   PRT_DENOISE_VAR_STATS    the {l, s2} plane of prt_render_adaptive with n = the pixel's paths: m = l / n, v = max((s2 - l m) / (n (n - 1)), 0)
 *                            (0 for n < 2).  Needs the last render since the reset to be prt_render_adaptive (else PRT_ERR_NOT_READY); for a
 *                            plain "N spp" picture with its plane render adaptively with min_spp = max_spp = N, rel_err = 0.
 *   PRT_DENOISE_VAR_SPATIAL  the unweighted 5x5 moments of L around the pixel, E[L^2] - E[L]^2 clamped at 0, window coordinates clamped into
 *                            the frame, non-finite colours left out
 *   PRT_DENOISE_VAR_AUTO     (default) stats when valid, else spatial.
 * Pass i = 0 .. passes-1, step s = 2^i:
 *   1. g = 3x3 Gaussian 1/16 [1 2 1; 2 4 2; 1 2 1] of v, coordinates clamped into the frame.
 *   2. Taps q = p + s (dx, dy), dx, dy in -2..2; taps outside the frame or with a non-finite colour are skipped.
 *        h   = k(dx) k(dy), k = (1/16, 1/4, 3/8, 1/4, 1/16)
 *        w_n = max(0, n_p.n_q)^sigma_n when both pixels have cov > 0; 1 when neither has; 0 when one has
 *        w_z = exp(-|z_p - z_q| / (sigma_z grad_p s sqrt(dx^2 + dy^2) + 1e-4)); grad_p = max over x and y of the absolute difference of z:
 *              central (|z(+1) - z(-1)| / 2) when both neighbours are in the frame with cov > 0, one-sided (|z(+-1) - z_p|) when one is,
 *              0 when none is or cov_p = 0
 *        w_a = exp(-|a_p - a_q|^2 / sigma_a^2)
 *        w_l = exp(-|L(c_p) - L(c_q)| / (sigma_l sqrt(g_p) + 1e-6))
 *        w = w_n w_z w_a w_l, except w = 1 for the centre tap (dx = dy = 0; what the product is for guides with a unit normal) and
 *        w = 0 where the product is NaN (a tap is dropped);   c' = sum h w c / sum h w;   v' = sum h^2 w^2 v / (sum h w)^2
 * Output: rgba with the framebuffer's alpha; a pixel whose own colour is not finite keeps it.  f32 arithmetic, deterministic (the same
 * inputs give the same bits).  prt_denoise reads the framebuffer, the state and the stats plane and writes none of them; `rgba` (may be NULL)
 * gets the filtered image in prt_read_framebuffer's layout, `rgba8` (may be NULL) prt_tonemap_rgba8's display transform of it.
 * Refused: PRT_ERR_NOT_READY without valid guides or without a render since the reset; PRT_ERR_UNSUPPORTED on tile and row-block contexts
 * (the filter needs the whole frame) and with a debug view; PRT_ERR_INVALID_ARGUMENT for passes outside 1..8, a sigma that is not > 0
 * (NaN included) or an unknown var_source.  params NULL = the defaults below. */
#define PRT_DENOISE_VAR_AUTO 0u
#define PRT_DENOISE_VAR_STATS 1u
#define PRT_DENOISE_VAR_SPATIAL 2u
#define PRT_DENOISE_DEFAULT_PASSES 5u
#define PRT_DENOISE_DEFAULT_SIGMA_L 3.0f      /* (4 moved a 4096-spp picture of cornell_mixed by relMSE 1.1e-3: DESIGN.md s4) */
#define PRT_DENOISE_DEFAULT_SIGMA_N 128.0f
#define PRT_DENOISE_DEFAULT_SIGMA_Z 1.0f
#define PRT_DENOISE_DEFAULT_SIGMA_A 0.1f
typedef struct prt_denoise_params {
    uint32_t passes;      /* 1 .. 8 */
    uint32_t var_source;  /* PRT_DENOISE_VAR_* */
    float sigma_l, sigma_n, sigma_z, sigma_a;
} prt_denoise_params;
int prt_denoise(prt_ctx* ctx, const prt_denoise_params* params, float* rgba, uint8_t* rgba8);

/* Temporal reprojection: the temporal part of SVGF (Schied et al. 2017) in front of prt_denoise's filter, for a moving camera (the reference
 * restarts accumulation from black on every camera move: src/main.cpp:283-291).  The intended loop per displayed frame: prt_set_camera,
 * prt_reset, render N spp with fresh seeds, prt_render_guides, prt_denoise_temporal.  For a still camera plain accumulation (no reset) plus
 * prt_denoise is the better path: the mean of all paths has less variance than any exponential average of it.
 * Inputs: the framebuffer colour c (the mean since the last prt_reset), the current guides {a, cov, n, z} and the history: per pixel
 * {c_h, n_h, m1, m2}, the guides of the previous call and its camera basis (DevCamera of camera_basis: P = position, M = middle,
 * Hz = horizontal, Vt = vertical).  At the end of each call the history takes the current guides and camera.  L(c) as in prt_denoise.
 *   World point of pixel p = (x, y): d = normalize(onPlane(p) - position), onPlane = create_cam_ray's expression at the pixel centre
 *     (sx = x / (W-1), sy = (H-1-y) / (H-1)), with the current camera.  cov_p > 0: X = position + z_p d -- the pinhole centre ray (with a
 *     lens an approximation; after a mirror or glass chain the virtual point behind the surface).  With a motion plane (prt_set_motion) and m_p > 0,
 *     D_p != 0: X + D_p, where that point of the mesh was, in its place.  cov_p = 0: the pixel reprojects as the
 *     direction d (a point at infinity).
 *   Projection into the previous camera: e = X - P (d for a direction); no history when dot(e, M - P) <= 0.  f = M - P,
 *     q = e dot(f, f) / dot(e, f) - f, a = dot(q, Hz) / dot(Hz, Hz), b = dot(q, Vt) / dot(Vt, Vt); x' = (a + 1)/2 (W-1),
 *     y' = (H-1) - (b + 1)/2 (H-1) (the inverse of create_cam_ray's centre ray); no history unless -1 < x' < W and -1 < y' < H.
 *   Taps: the 2x2 around (x', y'): x0 = floor(x'), y0 = floor(y'), fx = x' - x0, fy = y' - y0, bilinear weights (1-fx)(1-fy), fx (1-fy),
 *     (1-fx) fy, fx fy.  A tap t is valid when it lies in the frame, its stored colour is finite, the coverages agree (cov_p > 0 and
 *     cov_prev(t) > 0, or both 0) and, when covered, |z_prev(t) - |X - P|| <= tau_z |X - P| + grad_p (grad_p: prt_denoise's depth
 *     gradient of the current guides) and dot(n_p, n_prev(t)) >= cos_n.  No history when the sum w of the valid taps' weights is < 0.01, the
 *     history is empty or the point is behind the previous camera.
 *   Accumulation.  With history: c_h, m1_h, m2_h, n_h = the sums over the valid taps of w times the stored values, divided by sum w;
 *     n = min(n_h + 1, history_cap), ac = max(alpha_color, 1/n), am = max(alpha_moments, 1/n), c_i = c_h + ac (c - c_h),
 *     m1 = m1_h + am (L - m1_h), m2 = m2_h + am (L^2 - m2_h), L = L(c).  Without history: n = 1, c_i = c, m1 = L, m2 = L^2.  A pixel whose
 *     c is not finite keeps it: c_i = c, and its history restarts (n = 1).
 *   Variance: v = max(m2 - m1^2, 0) when n >= 4, else prt_denoise's v of the current frame for the var_source of `spatial`.
 *   Filter: {c_i, v} go through prt_denoise's passes unchanged, with the current guides; output as prt_denoise's (rgba with the framebuffer's
 *     alpha, rgba8 its display transform; either may be NULL).  The history stores n, m1, m2, v and the colour
 *       PRT_TEMPORAL_FEEDBACK_ATROUS      (default, SVGF) the output of a-trous pass 0
 *       PRT_TEMPORAL_FEEDBACK_INTEGRATED  c_i.
 * f32 arithmetic, deterministic, no atomics.  The call reads the framebuffer, the state, the stats plane and the guides and writes none of them.
 * History lifetime: allocated on first use (96 bytes per pixel); prt_reset and prt_set_camera keep it; prt_upload_scene, prt_upload_envmap,
 * prt_resize, prt_set_tile, prt_set_row_blocks and prt_reset_history empty it.  prt_read_history: per pixel 8 floats {c.rgb, n, m1, m2, v, 0},
 * framebuffer order; PRT_ERR_NOT_READY while the history is empty.
 * Refused as prt_denoise (NOT_READY without valid guides or without a render since the reset, UNSUPPORTED on tile and row-block contexts and
 * with a debug view), and PRT_ERR_INVALID_ARGUMENT for any parameter of either struct out of range or NaN or an unknown feedback.
 * NULL params = the defaults (the temporal ones are SVGF's). */
#define PRT_TEMPORAL_FEEDBACK_INTEGRATED 0u
#define PRT_TEMPORAL_FEEDBACK_ATROUS 1u
#define PRT_TEMPORAL_DEFAULT_ALPHA_COLOR 0.2f
#define PRT_TEMPORAL_DEFAULT_ALPHA_MOMENTS 0.2f
#define PRT_TEMPORAL_DEFAULT_TAU_Z 0.05f
#define PRT_TEMPORAL_DEFAULT_COS_N 0.9f
#define PRT_TEMPORAL_DEFAULT_HISTORY_CAP 32u
typedef struct prt_temporal_params {
    float alpha_color;     /* [0, 1]: blend floor of the colour; 0 = a plain running mean up to history_cap */
    float alpha_moments;   /* [0, 1] */
    float tau_z;           /* > 0: relative depth tolerance of a history tap */
    float cos_n;           /* [-1, 1]: minimum n_cur . n_prev of a history tap */
    uint32_t history_cap;  /* >= 1 */
    uint32_t feedback;     /* PRT_TEMPORAL_FEEDBACK_* */
} prt_temporal_params;
int prt_denoise_temporal(prt_ctx* ctx, const prt_denoise_params* spatial, const prt_temporal_params* temporal, float* rgba, uint8_t* rgba8);
int prt_read_history(prt_ctx* ctx, float* out8);
int prt_reset_history(prt_ctx* ctx);

/* Denoising a frame that was rendered in parts (tiles, row blocks, several devices): every part exports what the filter reads as records,
 * the caller puts the records of the whole frame together (parallel.py: one gather to rank 0) and the filter runs on them.  Moving records
 * is lossless, renders and guides are the same bits for every split of the frame and the filter is deterministic: the result is
 * prt_denoise's of a whole-frame context, bit for bit.
 * One record = PRT_DENOISE_RECORD_FLOATS floats (64 bytes) per pixel, framebuffer order:
 *   { c.r, c.g, c.b, alpha,   a.r, a.g, a.b, cov,   n.x, n.y, n.z, z,   v, has_stats, 0, 0 }
 * floats 0-3 the words of prt_read_framebuffer, 4-11 those of prt_read_guides, v the PRT_DENOISE_VAR_STATS variance above (the same f32
 * operations in the same order, 0 for n < 2) and has_stats = 1.0f when the last render since the reset was prt_render_adaptive; else v = 0 and
 * has_stats = 0.0f.
 * prt_export_denoise_inputs writes the records of the context's frame part (whole frame, tile or row blocks) to device memory of the caller
 * (width * rows records), ordered on the context's stream like prt_copy_framebuffer_to_device (complete on return unless the stream is a
 * caller's: prt_set_stream).  It reads the framebuffer, the state, the stats plane and the guides and writes none of them.  Refused as
 * prt_denoise, except that every frame part is served: PRT_ERR_NOT_READY without valid guides or without a render since the reset,
 * PRT_ERR_UNSUPPORTED with a debug view, PRT_ERR_INVALID_ARGUMENT for a null pointer or a context without a frame size.
 * prt_denoise_records runs prt_denoise's filter over a width x height frame given as width * height records in device memory, on the
 * context's device and stream.  It needs no scene, camera, frame size or render and uses scratch buffers of its own (grown on demand,
 * freed by prt_destroy): the context's frame, state, guides, stats plane and history are not touched, whatever size or part that frame is.
 *   Variance: PRT_DENOISE_VAR_SPATIAL the 5x5 moments of the records' colours; PRT_DENOISE_VAR_STATS the records' v (PRT_ERR_NOT_READY
 *   when any record has has_stats != 1); PRT_DENOISE_VAR_AUTO the records' v when every record has stats, else spatial.
 *   Output: `device_rgba` (may be NULL) width * height * 4 floats in device memory, `rgba` and `rgba8` (may be NULL) as prt_denoise's, in
 *   host memory; all complete on return.
 *   Refused: PRT_ERR_INVALID_ARGUMENT for width < 1, height < 1, null records, or parameters prt_denoise refuses.
 * prt_denoise_records_temporal is the same with prt_denoise_temporal's step in front.  `cam` is the camera the records were rendered with
 * (its basis as prt_set_camera derives it).  The record history (96 bytes per pixel, allocated on first use) is the context's second history:
 * prt_denoise_temporal's is another one, and nothing but prt_reset_records_history and a call with another width or height empties it (the
 * scene is the caller's here: reset it when the scene or the environment map changes).  A sequence of calls gives the bits of the same sequence
 * of prt_denoise_temporal on a whole-frame context.  Refused as prt_denoise_records and for parameters prt_denoise_temporal refuses;
 * PRT_ERR_INVALID_ARGUMENT for a null camera.
 * prt_read_records_history is prt_read_history's twin for the record history: after a synchronise, per pixel 8 floats {c.rgb, n, m1, m2, v, 0},
 * framebuffer order, of the width x height frame of the last prt_denoise_records_temporal call.  It writes nothing of the context.
 * PRT_ERR_NOT_READY while the record history is empty; PRT_ERR_INVALID_ARGUMENT for a null pointer or a size other than the history's. */
#define PRT_DENOISE_RECORD_FLOATS 16
int prt_export_denoise_inputs(prt_ctx* ctx, void* device_records);
int prt_denoise_records(prt_ctx* ctx, const prt_denoise_params* params, int width, int height, const void* device_records, void* device_rgba,
                        float* rgba, uint8_t* rgba8);
int prt_denoise_records_temporal(prt_ctx* ctx, const prt_denoise_params* spatial, const prt_temporal_params* temporal, const prt_camera* cam,
                                 int width, int height, const void* device_records, void* device_rgba, float* rgba, uint8_t* rgba8);
/* prt_denoise_records_temporal with the motion plane of the records' frame (width * height float4 {D, m} in device memory, 16-byte aligned:
 * the gathered prt_export_motion of every part).  device_motion NULL is exactly prt_denoise_records_temporal; both calls share the record history. */
int prt_denoise_records_temporal_motion(prt_ctx* ctx, const prt_denoise_params* spatial, const prt_temporal_params* temporal, const prt_camera* cam,
                                        int width, int height, const void* device_records, const void* device_motion, void* device_rgba,
                                        float* rgba, uint8_t* rgba8);
int prt_reset_records_history(prt_ctx* ctx);
int prt_read_records_history(prt_ctx* ctx, int width, int height, float* out8);

/* Pixel reconstruction filter of the primary rays: antialiasing (no counterpart in the reference, whose every path starts through the exact
 * pixel centre; opt-in, the default is that centre ray, bit for bit).  Filter importance sampling (Ernst et al. 2006): path k of pixel (x, y)
 * starts through (x + dx, y + dy), (dx, dy) drawn from a separable non-negative filter F(dx, dy) = f(dx) f(dy), every sample with weight 1 --
 * the framebuffer's mean estimates the filter-weighted pixel integral, and a pixel's estimate still depends on its own paths only (tiles,
 * row blocks, run-ahead, pacing, adaptive freezing, checkpoints keep their bits; no atomics, no splatting).
 *   Sample point of path k (0-based index of the path in its pixel since the last reset: samples - 1 after the path start counted it), global
 *   pixel coordinates, integer arithmetic mod 2^32:
 *       s = gy * 0x9E3779B9 + gx;   hx = lowbias32(s);   hy = lowbias32(s ^ 0x68E31DA4)
 *       lowbias32(v): v ^= v >> 16; v *= 0x7FEB352D; v ^= v >> 15; v *= 0x846CA68B; v ^= v >> 16
 *       ux = k * 3242174889 + hx;   uy = k * 2447445414 + hy                 (R2 in 0.32 fixed point, rotated per pixel)
 *       u = (float)(ux >> 8) * 2^-24,  v = (float)(uy >> 8) * 2^-24        (exact, in [0, 1));   dx = w(u), dy = w(v)
 *   It takes no draw from the path's RNG stream: apart from the ray direction every path keeps the reference's random sequence.
 *   The warp w, f32, no contraction, sqrtf correctly rounded:
 *       BOX              w(u) = (u - 0.5f) * (2r)
 *       TENT             w(u) = r * (sqrtf(2u) - 1) for u < 0.5f, else r * (1 - sqrtf(2 - 2u))
 *       GAUSSIAN         f(x) = exp(-x^2 / 2s^2) - exp(-r^2 / 2s^2), s = r / 3
 *       BLACKMAN_HARRIS  f(x) = 0.35875 + 0.48829 cos(pi x / r) + 0.14128 cos(2 pi x / r) + 0.01168 cos(3 pi x / r)
 *     the last two through a table T[0 .. 256] built when the filter is set: T[i] = F^-1(i / 256) in float64 rounded to f32, F the normalised
 *     CDF of f on [-r, r] in closed form, built antisymmetric (T[256 - i] = -T[i], T[128] = 0: w(0.5) = 0 exactly);
 *       t = u * 256.0f;  j = (int)t;  t -= j;  w = T[j] + t * (T[j+1] - T[j])
 *   Camera ray: create_cam_ray's expression at sx = (x + dx) / (W-1), sy = (H-1-y - dy) / (H-1) (the convention of the guides); the lens
 *   sample and the time draw are unchanged.
 *   Radius: 0 <= r <= 4, PRT_FILTER_DEFAULT_RADIUS = the kind's default; NaN, infinities, other negatives, values above 4 and unknown kinds:
 *   PRT_ERR_INVALID_ARGUMENT.  r = 0 is accepted for every kind: every ray goes through the centre, through the filter instances (bit-exact
 *   with PRT_FILTER_NONE: a plumbing check).
 *   Lifetime: a context starts with PRT_FILTER_NONE.  Setting a filter implies a reset of the frame (when it has one) and makes the guides stale;
 *   the temporal history is kept (as with prt_set_camera).  The filter survives prt_resize, prt_set_tile, prt_set_row_blocks, prt_upload_scene.
 *   Guides under a filter: guide sample s sits at the offset (w(fx), w(fy)) instead of (fx - 0.5, fy - 0.5) (the lens sample still comes from
 *   the unwarped (fx, fy)): box 0.5 gives the unfiltered guides bit for bit, K = 1 the centre for every filter.
 *   prt_render_frames, prt_render_spp, prt_render_adaptive and prt_render_guides honour it; the option "pool" is not used under a filter.
 *   Refused with PRT_ERR_UNSUPPORTED (no filter instances of these sets): a debug view, SDF primitives (geom_flags), pick_random_light,
 *   env_importance_sampling.
 * prt_pixel_filter_offsets needs no device and no context: out2 = {dx, dy} of paths k0 .. k0+n-1 (mod 2^32) of global pixel (gx, gy). */
#define PRT_FILTER_NONE 0u              /* default: the reference's pixel-centre ray (bit-exact, the existing kernels) */
#define PRT_FILTER_BOX 1u               /* default radius 0.5 */
#define PRT_FILTER_TENT 2u              /* default radius 1.0 */
#define PRT_FILTER_GAUSSIAN 3u          /* default radius 1.5, sigma = radius / 3 */
#define PRT_FILTER_BLACKMAN_HARRIS 4u   /* default radius 2.0 */
#define PRT_FILTER_DEFAULT_RADIUS (-1.0f)
int prt_set_pixel_filter(prt_ctx* ctx, uint32_t kind, float radius);
int prt_pixel_filter_offsets(uint32_t kind, float radius, uint32_t gx, uint32_t gy, uint32_t k0, uint32_t n, float* out2);

/* The sampling density of an environment map under prt_config::env_importance_sampling, as the cumulative tables prt_upload_envmap builds
 * for the kernels (no counterpart in the reference).  Needs no device and no context.  rgb: w x h float RGB texels, row 0 = the +y pole.
 *   lum(i, j)  = 0.2126 r + 0.7152 g + 0.0722 b of texel (i, j) in float64; 0 where that is not in (0, 1e30)
 *   m(i, j)    = the largest lum over the 3 x 3 neighbourhood of (i, j): columns wrap (i - 1 of column 0 is column w - 1), rows clamp
 *   s(j)       = sin(pi (j + 0.5) / h), the row centre's sin(theta)
 *   f(i, j)    = m(i, j) s(j) + 0.05 mean(m s) s(j) pi / 2        (the floor: 5 % of the mean, in proportion to the solid angle;
 *                                                                   a map without a positive texel: f = s(j) pi / 2)
 *   rows[j]    = sum of f over rows 0 .. j - 1 / sum of f,  j = 0 .. h          (rows[0] = 0, rows[h] = 1)
 *   cols[j (w + 1) + i] = sum of f(0 .. i - 1, j) / sum of f(., j),  i = 0 .. w   (0 .. 1 in every row)
 * summed in float64 in index order, each entry rounded to float32.  The density over directions inside texel (i, j), at polar coordinate
 * v = theta / pi, is (rows[j + 1] - rows[j]) (cols[j][i + 1] - cols[j][i]) w h / (2 pi^2 sin(pi v)): positive wherever the bilinear lookup of
 * the map can be. */
int prt_env_cdf(const float* rgb, int w, int h, float* rows /* h + 1 */, float* cols /* h * (w + 1) */);

/* Scheduling knob of the render kernel (no counterpart in the reference; results do not depend on it, tests check
 * that): a wave ends a BVH-walk phase once fewer than `lanes` of its 64 lanes are still walking (and fewer than wait for the
 * phase to end); the lanes cut off resume in the wave's next phase.  1 = every walk runs to its end (lock step).
 * Default: 8 (6 with a global medium and for launches with scattered pixels, 20 through big trees) for the closest-hit phases
 * (PRT_WALK_MIN_LANES); for the shadow rays' any-hit
 * phases 1 in small trees and 12 in big ones (PRT_SHADOW_MIN_LANES).  A call of this function sets both. */
int prt_set_walk_min_lanes(prt_ctx* ctx, uint32_t lanes);

/* Build and schedule choices of a context (no counterpart in the reference; NONE changes a bit of any result -- the tests render
 * the goldens under each).  For tests, experiments and tuning.  prt_create reads the same names from the environment, in upper
 * case with the prefix PRT_.
 *   "waves"             0 (default: chosen per launch) | 5 | 6   build of the render kernel: waves per SIMD its registers leave room for
 *   "scatter"           -1 (default: chosen per launch) | 0 | 1  a wave renders one 8x8 tile | 64 pixels scattered over the launch's tiles
 *   "generic"           0 | 1   1: the material set dispatched at run time even where the scene's own ACTIVE_MATS is compiled (the
 *                               reference compiles exactly the scene's set, include/CL/cl_kernel.h:226-345; compiled here: LIGHT|DIFF,
 *                               +COAT, +ROUGH_COND, +DIEL|ROUGH_DIEL)
 *   "any_dist"          0 | 1   1: the compiled set's instance that carries all three microfacet distributions even where every microfacet
 *                               lobe of the scene uses the same one (`mat->dist` is a run-time field in the reference,
 *                               kernels/bxdf/microfacet.cl:6-9; compiled here: GGX for the rough sets, Beckmann for the coat set)
 *   "walk_min_lanes", "shadow_min_lanes"   0 (by launch) .. 64   see prt_set_walk_min_lanes
 *   "tri_q"             0 .. 16  the triangle tests that a walk phase's box steps found run once this many sixteenths of its walking
 *                               lanes have one pending (default 4)
 *   "frames_per_launch" >= 0    frames one launch of the render kernel covers (0 = default: 512, or 4096 through a tree of more than 64 k node pairs)
 *   "run_ahead"         0 | 1   prt_render_spp: see there
 *   "pace"              1 | 0   prt_render_spp: a pixel whose paths are longer than the frame's average owes every launch proportionally more frames
 *                               (it needs proportionally more for its samples; what it does not do while the chip is full it does in the tail of the
 *                               render, alone); 0: every pixel owes a launch the same number of frames
 *   "tile_order"        1 | 0   prt_render_spp starts the tiles whose waves ran longest in a sub-part's first launch first in its later
 *                               launches (and renders, until scene, camera or frame change; setting the option to the value it has
 *                               keeps a measured order); 0: in index order
 *   "pix_per_wave"      0 (default: chosen per launch) | 64 | 32 | 16   pixels a wave of the render kernel renders (its other lanes idle).  Launches
 *                               that leave wave slots of the chip empty -- one rank's share of a frame split N ways, a small frame -- finish sooner
 *                               with more waves of fewer pixels: a wave lasts as long as the slowest of its pixels' chains of segments
 *   "pool"              0 | 1   1: render_kernel_rp (csrc/hip/pt_pool.h): workgroups of shading waves that post the rays that go deeper than the root
 *                               of the tree to walker waves through LDS.  Bit-exact, measured slower than the default kernel: off
 *   "compact"           1 | 0   prt_render_adaptive: list launches once few pixels are live (see there); 0: tiles to the end
 *   "compact_below"     0 .. 100   ... once fewer than this percentage of the frame's pixels are live (default 50); a list is rebuilt
 *                               once its live pixels have fallen below half of it
 *   "test_drop_report"  0 | 1   tests only: the launches of prt_render_spp and prt_render_adaptive report their unfinished pixels into a spare word, so that the
 *                               call sees a launch end without a report (PRT_ERR_HIP, state unusable until prt_reset) */
int prt_set_option(prt_ctx* ctx, const char* name, int value);

/* ---- Ray queries (no counterpart in the reference): closest hit, occlusion and pixel picking against the uploaded scene as it is NOW --
 * after every prt_update_vertices, prt_rebuild_bvh and prt_update_primitives -- without a render.  What is under the mouse (to choose the
 * sphere or the triangle to move), how far away the middle of the picture is (to set focalDistance), whether two points see each other.
 *
 * A cast sees exactly what a path segment of the render sees; the code is the render's (csrc/hip/pt_device.h, pt_cast.h):
 *
 * Closest hit, per valid ray:  limit = min(tmax, 20.0f)  (20 is the reference's INF, the farthest hit a ray of the render has);  ray_pre;
 *   walk_begin(sc, false, ray, limit, ...) and the walk run to its end;  finish_closest, with ray.normal = 0 before the call as the guides set it.
 *   The ray is a hit when the final t < limit.
 * Hit record:  t, pos, normal and backside (flags bit 0) are as finish_closest leaves them, the flip of the normal of a non-transmissive
 *   material towards the ray included (as in the reference, a triangle's material is looked up one record in front of the mesh table for
 *   this: in a scene whose config has a dielectric kind active the normal of a triangle hit is never turned, in every other scene it
 *   always faces the ray).  id is finish_closest's mesh id: i >= 0 = meshes[i] of the upload (a sphere, an SDF primitive or a
 *   quad), PRT_HIT_TRIANGLE for a triangle of the mesh.  For a triangle u, v are its barycentrics (the hit is p0 (1 - u - v) + p1 u + p2 v)
 *   and tri its index in the caller's vertex arrays -- vertices 3 tri .. 3 tri + 2, the number the refit tables hold for the slot
 *   (slot_vtx[slot] / 3): it survives prt_rebuild_bvh.  For every other kind of hit u, v and tri are 0.  A miss has id = PRT_HIT_MISS and
 *   every other word 0.
 * Directions:  the direction is used as given, it is not normalised, and t is in units of its length.  The triangle, box and quad tests
 *   hold for any length; the sphere and SDF tests assume a UNIT direction, as the render's rays have it.
 * Occlusion:  the render's shadow(): the any-hit walk with limit as above (1 = a triangle in (eps, limit)), and when the tree did not
 *   occlude, finish_shadow(origin, dir, limit): spheres, SDF primitives (shadow_marching_steps), quads.  eps = 1e-5.
 * Invalid rays:  a ray whose origin or direction has a non-finite component, whose direction is all zeros, or whose tmax is NaN or <= 0 is
 *   never walked: the casts report a miss for it, the occlusion tests 0.  The call itself succeeds.
 * prt_cast_pixels:  the ray of pixel (x, y), full-frame coordinates in framebuffer order (y as the rows of prt_read_framebuffer and of the guides): the centre ray of the pixel
 *   through the middle of the lens -- the guides' camera ray at offset 0 with the aperture point at the camera's position; for a pinhole
 *   camera sample 0 of prt_render_guides --, tmax = 20.  The rays are generated on the device and go through the same kernel.  Needs a
 *   camera and a frame size; a pixel outside [0, width) x [0, full_height) is reported as a miss.
 *
 * Every call reads the scene tables only.  It writes nothing of the context: path state, framebuffer, statistics plane, guides and their
 * validity, both histories, pending motion snapshots and measured tile orders stay as they are.  It is ordered on the context's stream and
 * complete on return, as prt_update_vertices_device is.  The host variants stage through buffers of the context, grown on demand and freed
 * by prt_destroy; the device variants take device memory, 16-byte aligned (rays: n x 32 bytes; hits: n x 48 bytes; out: n x 4 bytes).
 * Works on every uploaded tree, those prt_update_vertices refuses for their depth included, and needs neither camera nor frame size
 * (prt_cast_pixels does).
 * Refusals (the output is untouched):  PRT_ERR_NOT_READY without a scene, after a render call that failed half-way, and for prt_cast_pixels
 * without a camera or a frame size;  PRT_ERR_INVALID_ARGUMENT for a null pointer with n > 0, a misaligned device pointer and n > 2^26.
 * n == 0 succeeds and does nothing. */
#define PRT_HIT_MISS (-2)
#define PRT_HIT_TRIANGLE (-1)
typedef struct prt_ray { float origin[3]; float tmax; float dir[3]; float _pad; } prt_ray;   /* 32 bytes */
typedef struct prt_hit {                                                                      /* 48 bytes */
    float t, u, v; uint32_t tri;        /* tri: triangle index in the caller's vertex arrays (vertices 3 tri .. 3 tri + 2) */
    float normal[3]; int32_t id;        /* id: PRT_HIT_MISS (-2), PRT_HIT_TRIANGLE (-1), or i >= 0 = meshes[i] of the upload */
    float pos[3]; uint32_t flags;       /* bit 0: backside */
} prt_hit;
int prt_cast_rays(prt_ctx* ctx, const prt_ray* rays, uint32_t n, prt_hit* hits);                  /* host memory */
int prt_cast_rays_device(prt_ctx* ctx, const void* d_rays, uint32_t n, void* d_hits);             /* device memory, 16-byte aligned */
int prt_occluded(prt_ctx* ctx, const prt_ray* rays, uint32_t n, uint32_t* out);                   /* 1 = something in (eps, limit) */
int prt_occluded_device(prt_ctx* ctx, const void* d_rays, uint32_t n, void* d_out);
int prt_cast_pixels(prt_ctx* ctx, const int32_t* xy, uint32_t n, prt_hit* hits);                  /* n (x, y) pairs, full-frame coordinates */

/* Deforming geometry: the mesh POSED on the device from per-frame bone matrices -- linear blend skinning (no counterpart in the reference).
 * What an animated mesh changes per frame is a handful of 3x4 matrices: the caller gives the rest pose and the per-corner influences once
 * and from then on a few KB per frame; the library poses the 3T vertices (and normals) with one streaming kernel into buffers of the
 * context and hands them to the refit or the rebuild it already has.  A rigid part -- a door, a wheel, one group of an OBJ -- is a corner
 * with weights {1, 0, 0, 0}.  Opt-in: without these calls every bit of every result is what it was.
 * Corner c = 3i + k is vertex k of triangle i of prt_scene_desc::vertices.  Per corner: four bone indices b_0 .. b_3 (uint16) and four
 * weights w_0 .. w_3 (float).  A bone matrix M[b] is 12 floats, row-major 3x4: rows {m00 m01 m02 m03}, {m10 ..}, {m20 ..}.
 * The pose, all f32, no contraction; sqrtf and / correctly rounded.  Per corner with rest position (x, y, z), rest normal (nx, ny, nz), the
 * influences k = 0 .. 3 in that order:
 *       A_ij = +0                                               i = 0 .. 2, j = 0 .. 3
 *       for each k with w_k != 0:   A_ij = A_ij + w_k * M[b_k]_ij
 *     (a weight of +0 or -0 skips the influence, and its matrix is not read: it may hold NaN.  A rigid part costs one matrix.  A corner
 *     whose four weights are all zero goes to the origin.  Weights need not sum to 1 and may be negative.)
 *       p'.x = ((A00*x + A01*y) + A02*z) + A03;   p'.y and p'.z likewise with rows 1 and 2;   lane 3 = 0
 *       n'.x = (A00*nx + A01*ny) + A02*nz;        n'.y and n'.z likewise
 *       L = sqrtf((n'.x*n'.x + n'.y*n'.y) + n'.z*n'.z);     normal = L > 0 ? n' / L (per component) : n';     lane 3 = 0
 *     The normal is exact for blends of rotations with uniform scale and an approximation otherwise (the inverse transpose is out of scope:
 *     under a shear or a non-uniform scale regenerate the normals with prt_set_smooth_normals instead).  NaN and overflow go through the
 *     formulas as they stand.
 * The posed arrays go into buffers of the context, and the call proceeds EXACTLY as if those buffers had been passed to
 * prt_update_vertices_device (PRT_POSE_REFIT) or to prt_rebuild_bvh_device (PRT_POSE_REBUILD, max_leaf as there): its finite-vertex check
 * runs on the posed vertices -- a NaN or overflowing matrix under a non-zero weight is refused there, the scene untouched --, and the motion
 * snapshot rule, the guides going stale, the forgotten tile orders and what is kept are that path's.  With prt_set_smooth_normals on, or
 * with a skin without rest normals, normals == NULL is passed on: normals are then regenerated, kept or carried as that path defines.
 * Deterministic: no dependence between lanes, no atomics; tile, row-block and rank contexts that each set the same skin and pose stay
 * bit-identical in union to one whole-frame context.  The loop per displayed frame: pose, prt_reset, render, prt_render_guides,
 * prt_denoise_temporal.
 * prt_set_skin: checks and copies everything to the device and allocates the posed buffers and the matrix table (a pose cannot fail on an
 *   allocation after the scene has been touched).  Device memory per triangle: 48 bytes of rest vertices, 24 of indices, 48 of weights and
 *   48 of posed vertices -- 168 bytes --, with rest normals 48 + 48 more: 264 bytes; plus 48 bytes per bone.  Needs an uploaded scene with
 *   T > 0, else PRT_ERR_NOT_READY.  Refused with PRT_ERR_INVALID_ARGUMENT, each leaving the previous skin in force: a null rest_vertices,
 *   bone_index or bone_weight; n_bones outside 1 .. 65536; an index >= n_bones, even under a zero weight; a weight that is not finite; a
 *   rest x, y, z or normal component that is not finite (lane 3 is not looked at).  PRT_ERR_UNSUPPORTED for T > PRT_MAX_TRIANGLE_SLOTS.
 *   skin == NULL turns the feature off and frees the buffers.  Setting it changes no bit of the scene by itself.  It survives what the
 *   smoothing topology survives: prt_reset, prt_resize, tile and row-block calls, camera changes, updates, rebuilds and poses;
 *   prt_upload_scene turns it off (T may have changed).
 * prt_pose / prt_pose_device: `matrices` is n_bones x 12 floats -- host memory (copied to the context's table on its stream), or device
 *   memory of the context's device, 16-byte aligned.  Ordered on the context's stream and complete on return (the caller's matrices may be
 *   reused then).  PRT_ERR_NOT_READY without a skin; PRT_ERR_INVALID_ARGUMENT for null or misaligned matrices or an unknown mode; otherwise
 *   the refusals of the path it enters, each leaving the scene and a pending snapshot exactly as they were.
 * prt_read_posed: the posed buffers of the last pose, accepted or refused by its path: float4[3T] each.  PRT_ERR_NOT_READY before the first
 *   pose of the skin in force; PRT_ERR_INVALID_ARGUMENT for null `vertices`, or for non-null `normals` with a skin without rest normals. */
typedef struct prt_skin {
    const float*    rest_vertices;  /* float4[3T], layout of prt_scene_desc::vertices, xyz used */
    const float*    rest_normals;   /* float4[3T] or NULL */
    const uint16_t* bone_index;     /* 4 per corner */
    const float*    bone_weight;    /* 4 per corner */
    uint32_t        n_bones;        /* 1 .. 65536 */
    uint32_t        _pad;
} prt_skin;
#define PRT_POSE_REFIT   0u   /* then prt_update_vertices_device's path */
#define PRT_POSE_REBUILD 1u   /* then prt_rebuild_bvh_device's path, max_leaf as there */
int prt_set_skin(prt_ctx* ctx, const prt_skin* skin /* NULL = off, frees the buffers */);
int prt_pose(prt_ctx* ctx, const float* matrices /* n_bones x 12, host */, uint32_t mode, uint32_t max_leaf);
int prt_pose_device(prt_ctx* ctx, const void* d_matrices /* 16-byte aligned */, uint32_t mode, uint32_t max_leaf);
int prt_read_posed(prt_ctx* ctx, float* vertices /* float4[3T] */, float* normals /* float4[3T], may be NULL */);

/* Deforming geometry: the mesh MORPHED on the device from per-frame target weights -- morph targets / blend shapes, alone or in front of the
 * skin (no counterpart in the reference).  The second per-frame input of an animated mesh besides its bone matrices is a handful of
 * weights; the targets themselves are static, sparse per-corner deltas.  The caller gives the base mesh and the targets once and from then
 * on n_targets floats per frame; the library blends the 3T vertices (and normals) with one streaming kernel into buffers of the context and
 * hands them to the refit or the rebuild it already has -- or poses them by the skin in the same kernel (glTF's order: morph, then skin).
 * Opt-in: without these calls every bit of every result is what it was.
 * Corner c = 3i + k as for the skin.  A target lists the corners it moves, strictly ascending, with a position delta dp and -- optionally --
 * a normal delta dn per listed corner.  The ENTRIES of a corner are the (t, dp, dn) of every target t that lists it, in ascending t.
 * The morph, all f32, no contraction; sqrtf and / correctly rounded.  Per corner with base position (x, y, z) and base normal (nx, ny, nz):
 *       p = (x, y, z);   n = (nx, ny, nz)
 *       for each entry, in that order, with w = weights[t] != 0:     p.i = p.i + w * dp.i;   n.i = n.i + w * dn.i      i = x, y, z
 *     (a weight of +0 or -0 skips the entry.  A target with d_normal == NULL has dn = +0.  Weights need not sum to 1 and may be negative.)
 *   prt_morph:         vertex = {p, 0};   L = sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z);   normal = L > 0 ? n / L (per component) : n;  lane 3 = 0.
 *     A corner without an active entry keeps its base position bit for bit (a -0 stays -0: nothing is added) and gets its base normal
 *     renormalised by the same rule.
 *   prt_pose_morphed:  prt_pose's formulas exactly as they stand, with (x, y, z) = p and (nx, ny, nz) = n, un-normalised (the pose's own
 *     normalisation is the only one).  The skin's rest arrays are not read, the set's base takes their place: the result is that of prt_pose
 *     on a skin whose rest pose is p, n.  The morphed rest pose never goes to memory.
 *   NaN and overflow go through the formulas as they stand, and weights are not checked: a non-finite weight of a target that some corner
 *   lists gives a non-finite vertex, which the finite-vertex check of the entered path refuses, the scene untouched; of a target without
 *   entries it is harmless.
 * The morphed arrays go into buffers of the set (prt_morph) or into the skin's posed buffers (prt_pose_morphed: prt_read_posed returns them),
 * and the call proceeds EXACTLY as if those buffers had been passed to prt_update_vertices_device (PRT_POSE_REFIT) or to
 * prt_rebuild_bvh_device (PRT_POSE_REBUILD, max_leaf as there): the finite-vertex check, the motion snapshot rule, the guides going stale,
 * the forgotten tile orders and what is kept are that path's.  With prt_set_smooth_normals on, or with a set without base normals,
 * normals == NULL is passed on.  Deterministic: no dependence between lanes, no atomics; tile, row-block and rank contexts that each set the
 * same targets and morph stay bit-identical in union to one whole-frame context.
 * prt_set_morph_targets: checks, copies, builds the per-corner table on the host (a stable counting sort of the entries by corner) and
 *   allocates everything a morph will ever need, the morphed buffers and a table of n_targets weights included.  Device memory per triangle:
 *   48 bytes of base and 48 of morphed vertices, with base normals 48 + 48 more, and 12 bytes of offsets; per entry 16 bytes, with base
 *   normals 32; per target 4.  Needs an uploaded scene with T > 0, else PRT_ERR_NOT_READY.  Refused with PRT_ERR_INVALID_ARGUMENT, each
 *   leaving the set in force as it was: a null base_vertices or targets; n_targets outside 1 .. 65536; a target with n_entries > 0 and a null
 *   corner or d_position; a corner >= 3T or not strictly above its predecessor; a base x, y, z or normal component that is not finite; a delta
 *   component that is not finite (lane 3 is never looked at; d_normal is not read when the set has no base_normals).  PRT_ERR_UNSUPPORTED for
 *   T > PRT_MAX_TRIANGLE_SLOTS and for more than 2^32 - 1 entries in total.  set == NULL turns the feature off and frees the buffers.
 *   Setting it changes no bit of the scene by itself.  Its lifetime is the skin's: it survives prt_reset, prt_resize, tile and row-block
 *   calls, camera changes, updates, rebuilds, poses and morphs; prt_upload_scene turns it off.  It is independent of prt_set_skin, in both
 *   directions.
 * prt_morph / prt_morph_device: `weights` is n_targets floats -- host memory (copied to the set's table on the context's stream), or device
 *   memory of the context's device, 16-byte aligned.  mode and max_leaf as in prt_pose.  Ordered on the context's stream and complete on
 *   return.  PRT_ERR_NOT_READY without a set; PRT_ERR_INVALID_ARGUMENT for null or misaligned weights or an unknown mode; otherwise the
 *   refusals of the path it enters, each leaving the scene and a pending snapshot exactly as they were.
 * prt_pose_morphed / prt_pose_morphed_device: additionally PRT_ERR_NOT_READY without a skin, PRT_ERR_INVALID_ARGUMENT for null or misaligned
 *   matrices and when exactly one of the skin and the set has normals.
 * prt_read_morphed: the morphed buffers of the last prt_morph, accepted or refused by its path: float4[3T] each.  PRT_ERR_NOT_READY before
 *   the first one of the set in force; PRT_ERR_INVALID_ARGUMENT for null `vertices`, or for non-null `normals` with a set without base normals.
 * prt_set_morph_targets_layout: the same set under one of two table layouts; the morphed bits are the same under both, for every set and
 *   every weight vector, NaN and infinity included.  prt_set_morph_targets(ctx, set) is prt_set_morph_targets_layout(ctx, set,
 *   PRT_MORPH_LAYOUT_CORNERS).  A context has one set in force: either call replaces it, either call with set == NULL turns it off.  The
 *   refusals are prt_set_morph_targets', and an unknown layout is PRT_ERR_INVALID_ARGUMENT (tested after the scene, before set == NULL; the set
 *   in force stays).  The five morph doors and prt_read_morphed run over whichever table the set in force has.
 *   PRT_MORPH_LAYOUT_CORNERS: the per-corner table above.  A lane walks its corner's entries; a record holds its target's number, so it is
 *     loaded before its weight is known: the cost of a morph is that of all E entries whatever the weights are.
 *   PRT_MORPH_LAYOUT_PLANES: block b is corners 64 b .. 64 b + 63 (B = ceil(3T / 64) blocks, the last one may be ragged); a PLANE exists for
 *     every pair (target t, block b) where t lists at least one corner of b, the planes ordered by (b, t).  A plane is a 16-byte head
 *     {target, 0, the 64-bit mask of the listed lanes} and three rows of 64 floats (dp.x, dp.y, dp.z of lane l = c - 64 b; +0 on unlisted
 *     lanes), with base normals three more for dn.  A wave owns a block and reads each row as 256 contiguous bytes; a plane whose target's
 *     weight is zero costs the wave its head and its weight, two scalar loads, and no vector traffic: the cost of a morph is that of the
 *     planes of the targets with a non-zero weight.  A lane the mask does not list is left alone (nothing is added: a -0 stays -0, a NaN
 *     weight reaches listed lanes only), exactly as a corner without that entry is under CORNERS.
 * prt_get_morph_report: layout, n_targets, E = entries (the sum of n_entries), P = planes (0 under CORNERS) and table_bytes, the device bytes
 *   of the delta tables alone, with nrm = 1 with base normals, else 0:   CORNERS  4 (3T + 1) + 16 E (1 + nrm);
 *   PLANES  4 (B + 1) + 16 P + 768 P (1 + nrm).  (Either layout: 48 bytes per triangle of base and 48 of morphed vertices, with base normals
 *   48 + 48 more, and 4 per target, as above.)  The fill E / (64 P) is what to choose by: planes suit targets that are dense within the
 *   blocks they touch (a plane at fill f streams 12 / f + 0.25 / f bytes per entry against 16; but only those of active targets), corners
 *   suit scattered ones.  PRT_ERR_NOT_READY without a set in force, PRT_ERR_INVALID_ARGUMENT for a null `out`; it changes nothing. */
#define PRT_MORPH_LAYOUT_CORNERS 0u   /* prt_set_morph_targets' table: a CSR over corners */
#define PRT_MORPH_LAYOUT_PLANES  1u   /* per (target, block of 64 corners) one plane */
typedef struct prt_morph_target {
    const uint32_t* corner;      /* n_entries corner indices (c = 3i + k), STRICTLY ascending, each < 3T */
    const float*    d_position;  /* float4[n_entries], xyz used */
    const float*    d_normal;    /* float4[n_entries], xyz used; NULL = this target moves no normal (+0 deltas); not read when the set has no base_normals */
    uint32_t        n_entries;   /* 0 is allowed */
    uint32_t        _pad;
} prt_morph_target;
typedef struct prt_morph_set {
    const float* base_vertices;  /* float4[3T], layout of prt_scene_desc::vertices */
    const float* base_normals;   /* float4[3T] or NULL: no normals are morphed */
    const prt_morph_target* targets;
    uint32_t n_targets;          /* 1 .. 65536 */
    uint32_t _pad;
} prt_morph_set;
int prt_set_morph_targets(prt_ctx* ctx, const prt_morph_set* set /* NULL = off, frees the buffers */);
int prt_morph(prt_ctx* ctx, const float* weights /* n_targets, host */, uint32_t mode, uint32_t max_leaf);
int prt_morph_device(prt_ctx* ctx, const void* d_weights /* 16-byte aligned */, uint32_t mode, uint32_t max_leaf);
int prt_pose_morphed(prt_ctx* ctx, const float* matrices, const float* weights, uint32_t mode, uint32_t max_leaf);
int prt_pose_morphed_device(prt_ctx* ctx, const void* d_matrices, const void* d_weights, uint32_t mode, uint32_t max_leaf);
int prt_read_morphed(prt_ctx* ctx, float* vertices /* float4[3T] */, float* normals /* float4[3T], may be NULL */);
int prt_set_morph_targets_layout(prt_ctx* ctx, const prt_morph_set* set /* NULL = off */, uint32_t layout /* PRT_MORPH_LAYOUT_* */);
typedef struct prt_morph_report {
    uint32_t layout;       /* of the set in force */
    uint32_t n_targets;
    uint64_t entries;      /* sum of n_entries over the targets */
    uint64_t planes;       /* 0 for CORNERS */
    uint64_t table_bytes;  /* device bytes of the delta tables alone (formulas above) */
} prt_morph_report;
int prt_get_morph_report(prt_ctx* ctx, prt_morph_report* out);

/* Deforming geometry: the cost of the current tree, measured on the device, and a rule that rebuilds a refitted tree once it has degraded (no
 * counterpart in the reference).  A refit keeps the topology, so a mesh that moves far from the pose its tree was built for renders through
 * boxes that overlap more and more; the surface-area-heuristic cost says by how much, and a rebuild resets it.
 * The cost, f64, all operations as written, no contraction.  "Pair" k is inner node k of the library's own table: the inner nodes the root
 * reaches, each holding the boxes and the kinds of its two children (what prt_read_bvh returns, without the nodes nothing references).
 *   Box area, for a box stored as f32 min_x max_x min_y max_y min_z max_z:  e_i = (double)max_i - (double)min_i;  d_i = e_i > 0.0 ? e_i : 0.0
 *     (max(e_i, 0) in its comparison form);  A = 2.0 * ((d_x*d_y + d_y*d_z) + d_z*d_x).
 *   Term of pair k:  t_k = w_0 + w_1;  for an inner child w = 1.0 * A(its box), for a leaf child of primitive_count n > 0
 *     w = (double)n * A(its box), for an empty leaf w = +0.0 whatever its box.
 *   Sum S: the n terms t_0 .. t_(n-1) are padded with +0.0 to the next power of two and reduced by the complete binary tree over the pair
 *     index: level by level, s[i] = s[2i] + s[2i+1], until one value is left.  The shape is part of the contract: it makes every bit of S
 *     independent of block size, grid size and scheduling (there are no atomics and no hand-off between workgroups in the kernels).
 *   Inner root:  cost = (A(root) + S) / A(root), root = the root's box as prt_read_bvh_bounds defines node 0 (the union rule over pair 0).
 *   Leaf root of n triangles:  cost = w / A(root) with w as for a leaf child -- n for a box with area, NaN for one without.
 *   A(root) == 0 goes through as IEEE gives it: NaN or an infinity.
 * Up to the order of the sum this is the SAH cost of prt_read_bvh's tree: the sum over the inner nodes the root reaches of their area, plus the
 * sum over the leaves of area x primitive_count, over the root's area.  The result is a pure function of the pair table and the root's box:
 * tile, row-block and rank contexts that hold the same tree get the same bits.
 * prt_bvh_cost: the cost of the current tree -- uploaded, refitted or rebuilt -- into *cost.  One launch per 256-fold level of the sum (three
 *   for a tree of 400 k pairs), ordered on the context's stream and complete on return; 8 bytes come back.  It reads the scene's tables only:
 *   like the ray queries it changes nothing of the scene, the frame, the guides, the histories or a pending motion snapshot (its partial sums,
 *   8 bytes per 256 pairs, are allocated on first use).  It works on trees that prt_update_vertices refuses for their depth.
 *   PRT_ERR_NOT_READY without a scene or with T == 0, PRT_ERR_INVALID_ARGUMENT for a null pointer.
 * prt_set_rebuild_policy: opt-in; off (the default) every bit of every result is what it is without these calls, and the refit path launches
 *   nothing new.  Setting it measures the BASELINE: the cost of the tree as it is at that moment; the baseline is measured again at the end of
 *   every accepted rebuild while the policy is in force -- prt_rebuild_bvh[_device], PRT_POSE_REBUILD, or the policy's own.  From then on every
 *   call that goes through prt_update_vertices_device's path -- prt_update_vertices, and PRT_POSE_REFIT of prt_pose*, prt_morph* and
 *   prt_pose_morphed* -- first does exactly what it does without a policy, then costs the refitted tree, and when
 *       cost > (double)limit * baseline            (false for a NaN on either side: no rebuild)
 *   proceeds exactly as if the caller had then called prt_rebuild_bvh_device with the same vertex and normal arguments and the policy's
 *   max_leaf (the host variant: with its staged buffers; a pose or a morph: with its posed buffers; normals == NULL is passed on as NULL).
 *   Every bit of the scene, the generated normals, the motion snapshot and the lifetimes are those of that sequence of two calls.  If the
 *   rebuild is refused or fails, the call returns the rebuild's status and message, and the scene is the valid REFITTED one: the vertices
 *   have arrived, the old topology stays (e.g. normals == NULL under a caller's tree that does not reference every triangle: every update
 *   that passes the limit returns PRT_ERR_INVALID_ARGUMENT and leaves a scene that renders).
 *   limit: a factor >= 1 (1.3: rebuild once the refitted tree costs 30 % more than the last built one); max_leaf as prt_rebuild_bvh, 0 = its
 *   default.  policy == NULL turns it off.  Needs an uploaded scene with T > 0, else PRT_ERR_NOT_READY.  Refused with
 *   PRT_ERR_INVALID_ARGUMENT, each leaving the policy in force as it was: a limit that is not finite or below 1, max_leaf > 64.
 *   PRT_ERR_UNSUPPORTED where no rebuild could ever be accepted (T - 1 > PRT_MAX_NODE_PAIRS).  Setting it changes no bit of the scene.  It
 *   survives what the skin survives -- prt_reset, prt_resize, tile and row-block calls, camera changes, updates and rebuilds;
 *   prt_upload_scene turns it off.
 * prt_get_rebuild_report: what the last refit-path call under the policy did -- cost: the cost after its refit (before any such call: the
 *   baseline measured by prt_set_rebuild_policy); rebuilt: 1 if that call rebuilt; rebuilds: the rebuilds the policy has made since it was
 *   set; baseline: the baseline in force now (after that call, or after an explicit rebuild since).  PRT_ERR_NOT_READY without a policy,
 *   PRT_ERR_INVALID_ARGUMENT for a null pointer.
 * The loop per displayed frame with a policy: update (or pose, or morph), prt_reset, render, prt_render_guides, prt_denoise_temporal -- the
 * caller never reads the tree. */
typedef struct prt_rebuild_policy {
    float limit;           /* rebuild when cost > limit * baseline; finite, >= 1 */
    uint32_t max_leaf;     /* of the rebuild: 1 .. 64, 0 = the library's default */
} prt_rebuild_policy;
typedef struct prt_rebuild_report {
    double cost, baseline;
    uint32_t rebuilt;
    uint32_t rebuilds;
} prt_rebuild_report;
int prt_bvh_cost(prt_ctx* ctx, double* cost);
int prt_set_rebuild_policy(prt_ctx* ctx, const prt_rebuild_policy* policy /* NULL = off */);
int prt_get_rebuild_report(prt_ctx* ctx, prt_rebuild_report* out);

/* What this library was built from (no counterpart in the reference): a hash of the content of every source, header and compiler flag
 * of libprt.so, compiled in by the build (photorealistic-rendering-using-opencl_amd/build.py source_build_id(); a development variant of
 * tools/build_variant.sh reads "variant-<name>-<hash>").  bench.py prints it as `build_id` and refuses to time a library whose id is
 * not the working tree's; tests/conftest.py asserts the same.  Needs no device and no context. */
const char* prt_build_id(void);
/* what the last launch ran, as text: "render_kernel<LIGHT|DIFF> waves=6 pixels=tiles" ("" before the first launch; "pixels=scattered",
 * "pixels=tiles, expensive first": see prt_set_option; the pixel filter's builds: "render_kernel<LIGHT|DIFF,filter=tent> ...") */
const char* prt_kernel_variant(prt_ctx* ctx);

int prt_synchronize(prt_ctx* ctx);

/* output texture: linear float4 acc/samples per pixel (kernels/main.cl:159).  Row 0 is the BOTTOM of the
 * picture, as in the reference's GL texture (the camera maps coord.y = 0 to the lowest scan line,
 * kernels/camera.cl:29-35; its PNG writer flips on write, include/GL/cl_gl_interop.h:139). */
int prt_read_framebuffer(prt_ctx* ctx, float* rgba);
/* display side ("next" row N3): the reference's fragment shader (shaders/tonemapper.glsl:47-64: vignette,
 * filmic Reinhard with white point 1.2, smoothstep, gamma 2.2) applied on the device; 8-bit RGBA out, rows in
 * framebuffer order (what glReadPixels returns, include/GL/cl_gl_interop.h:147-150).  The vignette takes the pixel's
 * place in the whole frame: a tile or a row-block part gets its rows of the whole frame's picture.  Alpha is 255.
 * The transform is evaluated in float32, in the shader's order and without contraction, per channel x of the framebuffer:
 *     v = x * vignette;   q = 57.25f*v*v;   v = (q / (q + v + 56.25f)) / curve(1.2f);   t = clamp((v + 0.025f) / 1.025f, 0, 1);
 *     out = rint(255 * clamp(pow(t*t*(3 - 2*t), 1/2.2f), 0, 1))
 * with fmin / fmax that ignore a NaN operand.  So a NaN, +-inf and any value whose 57.25f*v*v overflows float32 (|x * vignette|
 * above about 2.4e18; q / (q + ...) is inf / inf there) map to 0 -- black, where exact arithmetic would say 255 for the large
 * ones --, and a zero of either sign and the denormals map to the byte of 0.0 (14 at the centre of the frame). */
int prt_tonemap_rgba8(prt_ctx* ctx, uint8_t* rgba);
/* same, device to device, into caller-owned device memory (e.g. a torch tensor).  Asynchronous on a stream given
 * with prt_set_stream (ordered with the caller's other work there); complete on return otherwise (the context's own
 * stream is private and non-blocking: nothing of the caller's is ordered against it). */
int prt_copy_framebuffer_to_device(prt_ctx* ctx, void* device_rgba);

/* r_flat, in the reference's 112-byte RTD layout (checkpoint / resume / parity checks), one record per pixel of this context's
 * frame part in framebuffer order.  The device keeps 80 bytes per pixel; of a record these are carried, bit for bit (floats as
 * their bits: NaN payloads, signed zeros and denormals included): origin[0..2], time, dir[0..2], dist, mask[0..2], total,
 * acc[0..3], samples, diff, spec, trans, scatters.  was_specular and reset are carried as flags: any non-zero value is read back
 * as 1.  origin[3], dir[3], mask[3] and the pad bytes are not carried: prt_write_state ignores them and prt_read_state returns
 * them as zero (as it does the converged bit of prt_render_adaptive, which no record shows).
 * prt_write_state also sets the framebuffer, as the render kernels leave it: acc[k] / (float)samples per channel (IEEE float32
 * division), and +0.0 in all four channels where samples == 0, whatever acc holds.  It leaves the context not fresh (prt_render_spp
 * and prt_render_adaptive need a prt_reset) and the adaptive statistics plane invalid. */
int prt_read_state(prt_ctx* ctx, prt_path_state* state);
int prt_write_state(prt_ctx* ctx, const prt_path_state* state);

/* run on a caller-provided hipStream_t (NULL = the context's own stream) */
int prt_set_stream(prt_ctx* ctx, void* hip_stream);

int prt_get_stats(prt_ctx* ctx, prt_stats* stats);
/* device-side reduction of samples / segments / frozen pixels (fills those prt_stats fields) */
int prt_query_counts(prt_ctx* ctx, uint32_t spp, prt_stats* stats);

/* Diagnostics: evaluates one function of include/prt_detmath.h ON THE DEVICE for n inputs
 * (fn: 0 sin, 1 cos, 2 tan, 3 exp, 4 log, 5 acos, 6 atan2(a,b), 7 pow(a,b), 8 sqrt, 9 a/b,
 * 10 fma(a,b,a), 11 fmin(a,b), 12 fmax(a,b), 13 round, 14 floor, 15 1/a, 16 cbrt).  Host arrays in and out.
 * The numerics contract says the result must equal the host evaluation bit for bit.
 * fn 17 - 19: the exhaustive checks of the kernels' exact fast paths (1/x, the quad's range test, sqrt; out = mismatches per lane).
 * fn 20 / 21: sin / cos of a through the kernels' one-evaluation pair helper; fn 22 / 23: the kernels' 1/a and sqrt(a) on the
 * caller's values (a wave = 64 consecutive inputs takes the IEEE expression as soon as one of them is outside the fast range);
 * fn 24: the quad's range test of x = a against the divisor c = b, 1.0 = outside [0, 1], with u = c * 2^-24 for 2^-40 <= c <= 2^40, NaN otherwise. */
int prt_selftest_math(prt_ctx* ctx, int fn, const float* a, const float* b, float* out, int n);
/* test hook: one device FUNCTION of the radiance loop on `n` cases (BSDF sampling / evaluation, microfacet terms,
 * Fresnel, light sampling, medium and phase sampling, camera ray, primitive tests, environment lookup -- fn 1..11, layouts in
 * csrc/hip/pt_selftest.h; fn 12: the pixel filter's offset, params {kind as uint bits, radius}, in {gx, gy, k as uint bits}, out {dx, dy},
 * csrc/hip/pt_filter.hip): 80 floats of shared parameters, 32 floats in and 32 floats out per case.  The known-answer
 * fixtures tests/golden/kat_*.npz hold what the REFERENCE's own functions return on the same cases.
 * fn 13 / 14: the environment-map importance sampling (not in the reference) on the map uploaded to a context created with
 * env_importance_sampling (PRT_ERR_INVALID_ARGUMENT without such a map); params is not read.  fn 13, env_sample: in {xi0, xi1}, out {d.xyz, pdf,
 * the texel i and j the search chose as uint bits, env_pdf(d), env_lookup(d).rgb}.  fn 14: in a direction, out {env_pdf, env_lookup.rgb}. */
int prt_selftest_fn(prt_ctx* ctx, int fn, const float* params, const float* in, float* out, int n);

const char* prt_last_error(prt_ctx* ctx);
/* message for a failed prt_create (ctx == NULL) */
const char* prt_last_global_error(void);

/* Temporal response: a second, short history beside each of the context's two histories and a clamp of the long one against it, for light
 * that changes on a surface that stands still (the "fast history" of ReLAX; variance clipping after Salvi 2016).  Such a tap passes every test
 * of the reprojection, so without the clamp a low alpha_color drags the old light for history_cap frames.  Opt-in: while the setting is off
 * (the default) every bit of every result of the temporal calls is what it is without it.  All f32, no contraction, no atomics.
 *   Fast history: one more colour f per pixel, double-buffered like the history (32 bytes per pixel per history, allocated by the first
 *     temporal call made with the setting on).  A pixel that takes the history branch (sum w >= 0.01) blends it from the same valid taps and
 *     weights:  f_h = (sum w f_prev) / sum w,  n_f = min(n_h + 1, fast_cap) with n_h the reprojected length before the + 1,
 *     f_i = f_h + (c - f_h) (1 / n_f).  A pixel without history, or with a non-finite c, takes f_i = c.  That is prt_denoise_temporal's accumulation with
 *     alpha_color = 0 and history_cap = fast_cap; it is never fed back from the filter (PRT_TEMPORAL_FEEDBACK_ATROUS touches the slow colour only).
 *   Clamp: a pass of its own behind the reprojection and in front of a-trous pass 0.  Window of pixel p: the taps q = p + (dx, dy) with
 *     |dx|, |dy| <= radius that lie in the frame and whose f_i(q) is finite in all three channels; m their number, taken dy outer and dx
 *     inner, both ascending.  Per channel: mu = (sum f) / m;  s = sum (f - mu)^2 (a second sweep, not E[f^2] - mu^2);  sigma = sqrtf(s / m);
 *     lo = mu - k sigma, hi = mu + k sigma.  When p took the history branch, its c_i is finite and m >= 1:
 *     c_i' = fminf(fmaxf(c_i, lo), hi) per channel, clamped = (c_i' != c_i in any channel), n' = clamped ? min(n, fast_cap) : n.
 *     The filter's input becomes {c_i', v} and the history stores {c_i', n'}; v, m1 and m2 stay as the reprojection made them (the moments of
 *     a pixel whose light just changed say "high variance", which is what the spatial filter should hear).  Every other pixel passes through
 *     bit for bit.
 *   prt_read_response / prt_read_records_response: per pixel 4 floats {f_i.rgb, flag} in framebuffer order, of the frame history / the record
 *     history; flag 0 = no history, 1 = history kept, 2 = clamped.  They write nothing.  PRT_ERR_NOT_READY while the setting is off or the
 *     history is empty; otherwise refused as prt_read_history / prt_read_records_history.  Those two keep returning 0 in float 7.
 *   prt_set_temporal_response: r NULL = off, which frees the fast planes.  A call that changes the setting empties both histories (the fast
 *     plane has nothing to reproject); a call with the values already in force does nothing.  Everything that empties a history empties its
 *     fast plane with it.  PRT_ERR_INVALID_ARGUMENT, leaving the setting in force, for fast_cap == 0, a radius outside 1 .. 3 or a k that is
 *     not > 0 or not finite; PRT_ERR_UNSUPPORTED with a debug view. */
#define PRT_RESPONSE_DEFAULT_FAST_CAP 4u
#define PRT_RESPONSE_DEFAULT_RADIUS 2u
#define PRT_RESPONSE_DEFAULT_K 2.0f
typedef struct prt_temporal_response {
    uint32_t fast_cap;   /* >= 1: length of the fast history in frames */
    uint32_t radius;     /* 1 .. 3: the window is (2 radius + 1)^2 pixels */
    float k;             /* > 0, finite: half-width of the clamp in sigmas */
    uint32_t _pad;
} prt_temporal_response;
int prt_set_temporal_response(prt_ctx* ctx, const prt_temporal_response* r);
int prt_read_response(prt_ctx* ctx, float* out4);
int prt_read_records_response(prt_ctx* ctx, int width, int height, float* out4);

#ifdef __cplusplus
}
#endif
#endif /* PRT_H */
