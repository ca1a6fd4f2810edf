// prt_ctx.h -- the context behind the C ABI of include/prt.h and what the prt_api*.cpp files that implement it share (internal: not
// installed).  Every device buffer of a context is a DevBuf (pt_devbuf.h) in one of three groups, by what it dies with: `scene` (replaced by
// prt_upload_scene), `frame` (replaced by prt_set_tile / prt_set_row_blocks) and `ctx` (prt_destroy alone).  Dropping a group is an
// assignment of a fresh one; bind() fills the pointers the kernels take (DevScene sc, DevState S) from the owners.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "prt.h"
#include "pt_devbuf.h"
#include "pt_launch.h"
#include "pt_layout.h"

using namespace prt;

// what a temporal call carries to the next one.  planes holds two halves of {c, n} and {m1, m2, v, 0} planes (half cur is the last call's,
// the other one is written by the next call: a flip of cur swaps them), guides the guides of the last call; cam its camera.  A history
// without one of its buffers is empty: only history_commit, which needs both, sets valid.  fast (prt_set_temporal_response): two halves of one
// {f.rgb, took the history branch} plane, flipped by the same cur; allocated by the first temporal call made with the setting on, it lives and
// dies with the history and is dropped when the setting goes off
struct History {
    DevBuf<float4> planes, guides, fast;
    int cur = 0;
    bool valid = false;
    DevCamera cam{};
};

// the tables of one tree (pt_refit.hip, pt_build.hip): a rebuild writes the spare set and swaps it with the live one.  root: the root's box
// (6 floats), then the check kernel's flag at word 6
struct TreeSet {
    DevBuf<NodePair> pairs;
    DevBuf<TriGeom> tri_geom;
    DevBuf<TriNrm> tri_nrm;
    DevBuf<uint32_t> slot_vtx, level_pairs;
    DevBuf<float> root;
};

// prt_set_motion: the triangle records (one per slot) and the primitive tables as they were before the first update since the last guide
// render, allocated by that update; *_valid: such a snapshot is pending -- the next prt_render_guides consumes it.  The two are independent
struct Snapshots {
    DevBuf<TriGeom> tri_prev;
    DevBuf<DevSphere> spheres_prev;
    DevBuf<DevSdf> sdfs_prev;
    DevBuf<DevQuad> quads_prev;
    bool snap_valid = false, prim_snap_valid = false;
};

// prt_set_smooth_normals (pt_normals.hip): the group of every corner, the group-to-members table, and what a generation writes -- the face
// buffer (face_r for the area weighting only) and the normals (float4[3T])
struct Smooth {
    DevBuf<uint32_t> group, first, member;
    DevBuf<float4> face_f, face_r;
    DevBuf<float> nrm;
    bool on = false;
    uint32_t weighting = 0;
    float crease = 0.0f;
};

// prt_set_skin (pt_pose.hip): the rest pose (float4[3T]; rest_n empty for a skin without normals), four indices and four weights per corner,
// the frame's matrices (12 floats per bone: the host door's staging) and what a pose writes -- the posed vertices and normals (float4[3T])
struct Skin {
    DevBuf<float> rest_v, rest_n, weight, mats, out_v, out_n;
    DevBuf<uint16_t> index;
    uint32_t n_bones = 0;
    bool on = false;
    bool posed = false;                            // a pose, accepted or refused, has written out_v (and out_n)
};

// prt_set_morph_targets (pt_morph.hip): the base mesh (float4[3T]; base_n empty for a set without normals), the per-corner table (offset
// [3T + 1], one float4 per entry and, with normals, a second one), the frame's weights (one float per target: the host doors' staging) and
// what prt_morph writes -- the morphed vertices and normals (float4[3T]).  Under PRT_MORPH_LAYOUT_PLANES the plane table takes the place of
// the per-corner one (pt_morph.h: block_first [ceil(3T / 64) + 1], a 16-byte head and 3 x 64 floats per plane and, with normals, 3 x 64
// more); entries and planes are the counts prt_get_morph_report returns
struct MorphSet {
    DevBuf<float> base_v, base_n, entry_p, entry_n, weights, out_v, out_n;
    DevBuf<uint32_t> offset;
    uint32_t layout = PRT_MORPH_LAYOUT_CORNERS;
    DevBuf<uint32_t> block_first;
    DevBuf<uint4> plane_head;
    DevBuf<float> plane_p, plane_n;
    uint64_t entries = 0, planes = 0;
    uint32_t n_targets = 0;
    bool on = false;
    bool morphed = false;                          // a prt_morph, accepted or refused, has written out_v (and out_n)
};

// prt_set_rebuild_policy (pt_cost.hip): the rule in force, the cost of the tree when the rule was set or a rebuild was last accepted, and
// what the last refit-path call under the rule did
struct RebuildPolicy {
    bool on = false;
    float limit = 0.0f;
    uint32_t max_leaf = 0;
    double baseline = 0.0;
    prt_rebuild_report rep{};
};

// everything of the uploaded scene: prt_upload_scene starts from a fresh one
struct Scene {
    TreeSet tree;                                  // slot_vtx, level_pairs and root arrive with the first update, query or rebuild (refit_tables)
    DevBuf<DevSphere> spheres;
    DevBuf<DevQuad> quads;
    DevBuf<DevSdf> sdfs;
    DevBuf<DevMaterial> mats;
    DevBuf<uint32_t> light_tab;
    // the host tables of the UPLOADED tree (PackedScene's): a rebuild empties slot_vtx, level_pairs and node_box -- its tables exist on the
    // device only -- and replaces level_first.  up_nodes / up_prims: the caller's tree, for prt_read_bvh; mesh_t: t of every prt_mesh
    std::vector<uint32_t> slot_vtx, level_pairs, level_first, node_box;
    std::vector<prt_bvh_node> up_nodes;
    std::vector<uint64_t> up_prims;
    std::vector<uint8_t> mesh_t;
    float root_bounds[6] = {0, 0, 0, 0, 0, 0};
    uint32_t n_tris = 0, n_nodes = 0;
    size_t n_slots = 0;                            // the slots of the current tree
    bool refit_ready = false;                      // tree.slot_vtx, level_pairs and root are there
    bool refitted = false;                         // an update has run since the upload: tree.root holds the root's box
    bool rebuilt = false;                          // the tree is a rebuilt one (node 0 the root, the children of pair k nodes 2k + 1 and 2k + 2)
    DevBuf<float> stage_vtx, stage_nrm;            // the host variants' vertices and normals (3 T float4 each), on first use
    // prt_update_primitives (pt_prims.hip), all by the first update: prim_types {the pack kernel's flag word, 12 bytes of padding, mesh_t}, the
    // staging tables the pack kernel writes (sized as the live ones) and the host variant's records
    DevBuf<unsigned char> prim_types;
    DevBuf<DevSphere> stage_spheres;
    DevBuf<DevSdf> stage_sdfs;
    DevBuf<DevQuad> stage_quads;
    DevBuf<prt_mesh> stage_meshes;
    Snapshots snap;                                // also dropped by prt_set_motion(off)
    Smooth smooth;                                 // also dropped by prt_set_smooth_normals(NULL)
    Skin skin;                                     // also dropped by prt_set_skin(NULL)
    MorphSet morph;                                // also dropped by prt_set_morph_targets(NULL)
    DevBuf<double> cost_work;                      // prt_bvh_cost's partials (cost_work_doubles of the pairs), on first use; grown when a rebuild needs more
    RebuildPolicy policy;                          // also dropped by prt_set_rebuild_policy(NULL)
};

// everything of the frame part, with its size: alloc_frame starts from a fresh one.  All but the state planes, fb and the tile buffers are
// allocated on first use
struct Frame {
    static constexpr int MAX_SUB = 4;              // the most sub-parts a frame part is rendered in (prt_ctx::n_sub)
    DevBuf<float4> q0, q1, q2, q3;                 // DevState
    DevBuf<uint4> q4;
    DevBuf<float4> fb;
    // prt_render_adaptive: the per-pixel plane {l, s2} and the live-pixel list (with ceil(npix / 64) + 1 words for the wave offsets and the count)
    DevBuf<float2> adapt;
    DevBuf<uint32_t> live, live_aux;
    bool stats_valid = false;                      // the last render since prt_reset was prt_render_adaptive: adapt belongs to the framebuffer
    // prt_render_guides / prt_denoise (pt_denoise.hip): the guide plane (2 float4 per pixel), the motion plane ({D, m} per pixel) and the
    // filter's buffers (frame_planes)
    DevBuf<float4> guides, motion;
    bool guides_valid = false;                     // cleared by everything that changes what a primary ray sees (prt.h)
    bool motion_valid = false;                     // motion was written by the guide render that made guides_valid
    DevBuf<float4> dn;
    DevBuf<float> dn_g;
    History hist;                                  // prt_denoise_temporal; hist.valid is cleared by everything prt.h lists
    // Expensive tiles first (prt_render_spp through trees of more than 64 k node pairs, FrameArgs::tile_order): the waves of launch 0 of
    // each sub-part leave what their tile cost (iterations),
    // the host sorts, and from launch 1 on -- and in later renders, until scene, camera or frame change -- the sub-part's workgroups take
    // their tiles in that order.  A launch ends with its last tile; started last, an expensive one keeps the launch open alone.
    DevBuf<uint32_t> tile_order[MAX_SUB], tile_cost[MAX_SUB];
    bool have_order[MAX_SUB] = {false, false, false, false};
};

// what only prt_destroy frees
struct CtxBuffers {
    DevBuf<float> env, env_rows, env_cols;         // the environment map and its two CDF tables survive scene uploads
    int env_w = 0, env_h = 0;
    DevBuf<int32_t> seeds;                         // grown on demand
    DevBuf<unsigned long long> counters;           // [0] unfinished, [1..3] count_kernel, [4 + 2j, 5 + 2j] {unfinished, waves done} of sub-part j
    DevBuf<float> filter_tab;                      // prt_set_pixel_filter: the table T[0 .. 256] of the Gaussian and Blackman-Harris kinds, on first use
    // prt_denoise_records (pt_records.hip): one block for a frame given as records -- its framebuffer plane, guide planes (2), the filter's
    // buffers (3), the Gaussian of v and the "a record without stats" word.  Grown on demand
    DevBuf<unsigned char> rec;
    History rec_hist;                              // prt_denoise_records_temporal: of a rec_hist_w x rec_hist_h frame, anew with every new size
    int rec_hist_w = 0, rec_hist_h = 0;
    // prt_cast_rays / prt_occluded / prt_cast_pixels (pt_cast.hip): the host variants' rays (32 bytes each; prt_cast_pixels puts its (x, y)
    // pairs behind the rays it generates) and results (48 bytes each).  Grown on demand
    DevBuf<unsigned char> cast_rays, cast_out;
    // prt_rebuild_bvh (pt_build.hip): the set the next tree is built into (and the snapshot in its slot order, with motion on), grown when a
    // new T needs more, and the build's scratch (bw over build_T triangles, laid out again whenever T differs).  They OUTLIVE the scene:
    // nothing in them is read before it is written (tests/test_call_sequences.py: uploads of fewer and of more triangles between rebuilds)
    TreeSet spare;
    DevBuf<TriGeom> spare_prev;
    DevBuf<unsigned char> build;
    uint32_t build_T = 0;
    BuildWork bw{};
};

struct prt_ctx {
    int device = 0;
    prt_config cfg{};
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing_pending = false;
    Scene scene;
    Frame frame;
    CtxBuffers ctx;
    DevScene sc{};                                 // what the kernels take: the scene's scalars, and the pointers bind() fills
    DevState S{};
    bool motion = false;                           // prt_set_motion
    bool response_on = false;                      // prt_set_temporal_response: the setting in force, of both histories
    prt_temporal_response response{};
    bool have_scene = false, have_cam = false, have_size = false;
    bool state_undefined = false;   // a render call failed half-way (prt_render_spp's abort path): pixels may be ahead of the launch windows
                                    // (run-ahead leads in the state) -- the state is unusable until prt_reset / prt_write_state
    DevCamera cam{};
    int width = 0, full_height = 0, row0 = 0, rows = 0;
    int block_rows = 1, n_parts = 1, part = 0;
    size_t npix = 0;
    // The megakernel renders the frame as n_sub interleaved sets of tiles, each on its own stream: the sets are
    // independent (pixels are), so while one set's launch drains on its slowest tiles the other fills the CUs.
    static constexpr int MAX_SUB = Frame::MAX_SUB;
    int n_sub = 2;
    bool n_sub_forced = false;      // PRT_STREAMS given: sub_parts does not fall back to one launch for small frames
    hipStream_t sub_stream[MAX_SUB] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t sub_ev[MAX_SUB] = {};              // end of a sub-part's launch (one in flight per sub-part)
    hipEvent_t sub_ev0[MAX_SUB] = {};             // its start (prt_render_spp times every launch)
    hipEvent_t fork_ev = nullptr;
    unsigned long long* h_unfinished = nullptr;   // pinned, [MAX_SUB] + a spare word: written by the last wave of a launch
    // frames a launch of render_kernel covers (PRT_FRAMES_PER_LAUNCH).  Lanes drift apart in frame number inside a launch
    // and the wave waits for its last lane at the end of each: long launches amortise that (cornell 1080p, MI355X:
    // 128 -> 7.85, 256 -> 8.18, 512 -> 8.33, 1024 -> 8.38, 2048 -> 8.08 G segments/s; 2 x 100 ms launches in flight at 512)
    // Through a tree beyond one XCD's L2 the lanes of a wave drift much further apart (deep walks), and every launch boundary makes a wave
    // wait for its slowest lane: 871 k triangles at 3840x2160, 512 spp: 512 -> 3.44, 1024 -> 3.57, 2048 -> 3.75, 4096 -> 3.84, 8192 -> 3.82 G
    // segments/s (a launch of 4096 frames of that scene runs 7.5 s; cornell: 256 -> 12.74, 512 -> 12.85, 1024 -> 12.66).
    // 0 = by tree size: 512, or 4096 beyond 64 k node pairs.
    unsigned frames_per_launch = 0;
    // walk phases end below this many walking lanes (prt_set_walk_min_lanes, PRT_WALK_MIN_LANES; 0 = chosen per launch, pt_kernels.hip
    // launch_variant_w).  Round-2 kernel at 4 waves: 1 -> 7.78, 4 -> 8.33, 6 -> 8.37, 8 -> 8.28, 12 -> 7.98 G segments/s; at 5 waves:
    // 4 -> 10.65, 6 -> 11.36, 8 -> 11.45, 12 -> 11.4
    uint32_t walk_min_lanes = 0;
    uint32_t shadow_min_lanes = 0;                 // the same for the shadow rays' walk phases (PRT_SHADOW_MIN_LANES; 0 = by tree size)
    // the pending triangle tests of a walk phase run once this many sixteenths of its walking lanes have one (PRT_TRI_Q; render_kernel)
    uint32_t tri_sixteenths = 4;
    uint32_t run_ahead = 1;                        // FrameArgs::run_ahead of prt_render_spp's launches (PRT_RUN_AHEAD=0: off)
    // prt_render_spp: pixels whose paths are longer than the frame's average owe every launch proportionally more frames (FrameArgs::pace_inv_ref;
    // PRT_PACE=0 / option "pace": off).  The frame's mean path length is taken once per render, after the first launch that retires.
    int pace = 1;
    int tile_sort = 1;                             // PRT_TILE_ORDER=0 / option "tile_order": off (Frame::tile_order)
    std::vector<uint32_t> h_tile_cost, h_tile_order;
    bool launch_log = false;                       // PRT_LAUNCH_LOG=1: one line per retired launch on stderr
    bool test_drop_report = false;                 // option "test_drop_report" (tests only): the launches of prt_render_spp and prt_render_adaptive report into a spare word
    prt_stats stats{};
    std::string err;
    LaunchOpts lo{};                               // forced wave-count build / pixel mapping / generic material set (prt_set_option)
    RenderLaunch last{};                           // what the last launch ran
    RenderLaunch last_sub[MAX_SUB] = {};           // ... per sub-part (their grids differ by up to one tile: so can the pixel mapping)
    std::string variant;                           // ... as text (prt_kernel_variant)
    bool fresh = false;                            // nothing rendered since prt_reset (or the frame's allocation)
    int compact = 1;                               // option "compact": list launches once few pixels are live
    int compact_below = 50;                        // option "compact_below": ... fewer than this percentage of the frame
    prt_adaptive_report arep{};                    // what the last adaptive render did with its launches
    // prt_set_pixel_filter: the kind and its radius.  Every launch carries them in FrameArgs
    uint32_t filter_kind = PRT_FILTER_NONE;
    float filter_r = 0.0f;
};

#define CTX_CHECK(ctx) do { if (!(ctx)) return PRT_ERR_INVALID_ARGUMENT; } while (0)
#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
        (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return PRT_ERR_HIP; } } while (0)

inline int fail(prt_ctx* ctx, int code, const std::string& msg) { ctx->err = msg; return code; }

// the pointers of sc and S from their owners: after everything that allocates, swaps or drops one of them (upload, rebuild, map upload,
// frame allocation)
inline void bind(prt_ctx* c) {
    const TreeSet& t = c->scene.tree;
    DevScene& sc = c->sc;
    sc.pairs = t.pairs; sc.tri_geom = t.tri_geom; sc.tri_nrm = t.tri_nrm;
    sc.spheres = c->scene.spheres; sc.quads = c->scene.quads; sc.sdfs = c->scene.sdfs; sc.mats = c->scene.mats; sc.light_tab = c->scene.light_tab;
    sc.env = c->ctx.env; sc.env_w = c->ctx.env_w; sc.env_h = c->ctx.env_h; sc.env_cdf_rows = c->ctx.env_rows; sc.env_cdf_cols = c->ctx.env_cols;
    const Frame& f = c->frame;
    c->S.q0 = f.q0; c->S.q1 = f.q1; c->S.q2 = f.q2; c->S.q3 = f.q3; c->S.q4 = f.q4;
}

// a check kernel's verdict before anything live is overwritten: the n flag words at `flags` (device) are cleared, `launch` queues the
// kernels that set them, and they are in `out` when this returns
template <typename Launch>
int checked(prt_ctx* c, uint32_t* flags, uint32_t* out, size_t n, Launch launch) {
    HIPCHK(c, hipMemsetAsync(flags, 0, n * sizeof(uint32_t), c->stream));
    launch();
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, flags, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// measured tile orders are the scene's, the view's and the frame's: whatever changes one of them forgets them
inline void forget_tile_orders(prt_ctx* c) { for (bool& h : c->frame.have_order) h = false; }

// the tables of the uploaded tree on the device -- slot_vtx, level_pairs, the root's box -- unless an update or a rebuild has put them there
// (prt_api_scene.cpp; the ray queries share slot_vtx with the refit)
int refit_tables(prt_ctx* c);

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int ready(prt_ctx* c, const char* who) {
    if (c->state_undefined) return fail(c, PRT_ERR_NOT_READY, std::string(who) + ": an earlier render call failed half-way; prt_reset or prt_write_state first");
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, std::string(who) + ": no scene uploaded");
    if (!c->have_cam) return fail(c, PRT_ERR_NOT_READY, std::string(who) + ": no camera set");
    if (!c->have_size) return fail(c, PRT_ERR_NOT_READY, std::string(who) + ": no frame size set");
    return PRT_OK;
}

inline FrameArgs frame_args(prt_ctx* c, uint32_t first_frame, uint32_t n, const int32_t* d_seeds, uint32_t spp, bool count) {
    FrameArgs fa;
    fa.width = c->width; fa.full_height = c->full_height; fa.row0 = c->row0; fa.rows = c->rows;
    fa.block_rows = c->block_rows; fa.n_parts = c->n_parts; fa.part = c->part;
    fa.first_frame = first_frame; fa.n_frames = n; fa.seed_pairs = d_seeds; fa.spp_limit = spp;
    fa.seed_frames = n; fa.run_ahead = 0; fa.pace_inv_ref = 0.0f;
    fa.unfinished = count ? c->ctx.counters.get() : nullptr;
    fa.unfinished_host = nullptr;
    fa.tile_first = 0; fa.tile_stride = 1; fa.scatter = 0; fa.sub_shift = 0;
    fa.tile_order = nullptr; fa.tile_cost = nullptr;
    // 0 = by launch (pt_kernels.hip launch_variant_w: the scattered-pixel launches and the medium variants 6, the others 8; shadow
    // phases in lock step in small trees, bounded like the closest-hit phases in big ones)
    fa.walk_min_lanes = c->walk_min_lanes;
    fa.shadow_min_lanes = c->shadow_min_lanes;
    fa.tri_sixteenths = c->tri_sixteenths;
    fa.adapt = nullptr; fa.live = nullptr; fa.live_count = 0;             // (prt_render_adaptive sets them: every other launch is "N spp" / frame mode)
    fa.min_spp = 0; fa.rel_err = 0.0f; fa.abs_floor = 0.0f;
    fa.filter_kind = c->filter_kind; fa.filter_r = c->filter_r;
    fa.filter_tab = c->filter_kind >= PRT_FILTER_GAUSSIAN ? c->ctx.filter_tab.get() : nullptr;
    return fa;
}
