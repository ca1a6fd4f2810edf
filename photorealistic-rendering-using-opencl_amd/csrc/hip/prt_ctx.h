// prt_ctx.h -- the context behind the C ABI of include/prt.h and what the files that implement it share (internal: not installed).
// The entry points by call group: prt_api.cpp (context, frame, camera, map, options, read-backs, selftests), prt_api_scene.cpp (upload,
// refit, rebuild), prt_api_render.cpp (the render drivers, guides, motion), prt_api_denoise.cpp (the filter, both histories, the records),
// prt_api_query.cpp (ray queries).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "prt.h"
#include "pt_launch.h"
#include "pt_layout.h"

using namespace prt;

// what a temporal call carries to the next one, allocated on first use.  planes holds two halves of {c, n} and {m1, m2, v, 0} planes (half
// cur is the last call's, the other one is written by the next call: a flip of cur swaps them), guides the guides of the last call; cam its
// camera
struct History {
    float4* planes = nullptr;
    float4* guides = nullptr;
    int cur = 0;
    bool valid = false;
    DevCamera cam{};
};

struct prt_ctx {
    int device = 0;
    prt_config cfg{};
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing_pending = false;
    // scene
    DevScene sc{};
    void* d_pairs = nullptr; void* d_tri_geom = nullptr; void* d_tri_nrm = nullptr;
    void* d_spheres = nullptr; void* d_quads = nullptr; void* d_sdfs = nullptr; void* d_mats = nullptr; void* d_light_tab = nullptr; void* d_env = nullptr; void* d_env_rows = nullptr; void* d_env_cols = nullptr;
    bool have_scene = false, have_cam = false, have_size = false;
    bool state_undefined = false;   // a render call failed half-way (prt_render_spp's abort path): pixels may be ahead of the launch windows
                                    // (run-ahead leads in the state) -- the state is unusable until prt_reset / prt_write_state
    DevCamera cam{};
    // frame
    int width = 0, full_height = 0, row0 = 0, rows = 0;
    int block_rows = 1, n_parts = 1, part = 0;
    size_t npix = 0;
    DevState S{};
    float4* fb = nullptr;
    int32_t* d_seeds = nullptr; size_t seeds_cap = 0;
    unsigned long long* d_counters = nullptr;     // [0] unfinished, [1..3] count_kernel, [4 + 2j, 5 + 2j] {unfinished, waves done} of sub-part j
    // The megakernel renders the frame as n_sub interleaved sets of tiles, each on its own stream: the sets are
    // independent (pixels are), so while one set's launch drains on its slowest tiles the other fills the CUs.
    static constexpr int MAX_SUB = 4;
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
    // Expensive tiles first (prt_render_spp through trees of more than 64 k node pairs, FrameArgs::tile_order): the waves of launch 0 of
    // each sub-part leave what their tile cost (iterations),
    // the host sorts, and from launch 1 on -- and in later renders, until scene, camera or frame change -- the sub-part's workgroups take
    // their tiles in that order.  A launch ends with its last tile; started last, an expensive one keeps the launch open alone.
    int tile_sort = 1;                             // PRT_TILE_ORDER=0 / option "tile_order": off
    uint32_t* d_tile_order[MAX_SUB] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t* d_tile_cost[MAX_SUB] = {nullptr, nullptr, nullptr, nullptr};
    bool have_order[MAX_SUB] = {false, false, false, false};
    std::vector<uint32_t> h_tile_cost, h_tile_order;
    bool launch_log = false;                       // PRT_LAUNCH_LOG=1: one line per retired launch on stderr
    bool test_drop_report = false;                 // option "test_drop_report" (tests only): the launches of prt_render_spp and prt_render_adaptive report into a spare word
    prt_stats stats{};
    std::string err;
    LaunchOpts lo{};                               // forced wave-count build / pixel mapping / generic material set (prt_set_option)
    RenderLaunch last{};                           // what the last launch ran
    RenderLaunch last_sub[MAX_SUB] = {};           // ... per sub-part (their grids differ by up to one tile: so can the pixel mapping)
    std::string variant;                           // ... as text (prt_kernel_variant)
    // prt_render_adaptive: the per-pixel plane {l, s2} and the live-pixel list (with ceil(npix / 64) + 1 words for the wave offsets and the
    // count), allocated on first use with the frame's size, freed with the frame
    float2* d_adapt = nullptr;
    uint32_t* d_live = nullptr;
    uint32_t* d_live_aux = nullptr;
    bool fresh = false;                            // nothing rendered since prt_reset (or the frame's allocation)
    int compact = 1;                               // option "compact": list launches once few pixels are live
    int compact_below = 50;                        // option "compact_below": ... fewer than this percentage of the frame
    prt_adaptive_report arep{};                    // what the last adaptive render did with its launches
    bool stats_valid = false;                      // the last render since prt_reset was prt_render_adaptive: d_adapt belongs to the framebuffer
    // prt_render_guides / prt_denoise (pt_denoise.hip): the guide plane (2 float4 per pixel) and the filter's buffers (two ping-pong planes,
    // the output plane, the Gaussian of v), allocated on first use with the frame's size, freed with the frame
    float4* d_guides = nullptr;
    bool guides_valid = false;                     // cleared by everything that changes what a primary ray sees (prt.h)
    float4* d_dn = nullptr;
    float* d_dn_g = nullptr;
    // prt_denoise_temporal (pt_temporal.hip): the history, allocated on first use with the frame's size, freed with the frame; hist.valid is
    // cleared by everything prt.h lists
    History hist;
    // prt_set_pixel_filter: the kind, its radius and, for the Gaussian and Blackman-Harris kinds, the table T[0 .. 256] on the device (allocated on
    // first use).  Every launch carries them in FrameArgs
    uint32_t filter_kind = PRT_FILTER_NONE;
    float filter_r = 0.0f;
    float* d_filter_tab = nullptr;
    // prt_denoise_records (pt_records.hip): one block for a frame of rec_cap pixels given as records -- its framebuffer plane, guide planes (2),
    // the filter's buffers (3), the Gaussian of v and the "a record without stats" word.  Not the context's frame: grown on demand, freed by
    // prt_destroy alone
    float4* d_rec = nullptr;
    size_t rec_cap = 0;
    // prt_denoise_records_temporal: the record history of a rec_hist_w x rec_hist_h frame, allocated on first use and with every new size,
    // emptied by prt_reset_records_history, freed by prt_destroy
    History rec_hist;
    int rec_hist_w = 0, rec_hist_h = 0;
    // prt_update_vertices (pt_refit.hip): the topology tables of the uploaded tree (host, PackedScene's), their device copies and the
    // root's box + flag word (d_refit_root: 6 floats, then the check kernel's flag at word 6), uploaded with the first update; the host
    // variant's staging buffers (3 T float4 each), allocated on first use.  All freed with the scene
    std::vector<uint32_t> slot_vtx, level_pairs, level_first, node_box;
    float root_bounds[6] = {0, 0, 0, 0, 0, 0};
    uint32_t n_tris = 0, n_nodes = 0;
    void* d_slot_vtx = nullptr; void* d_level_pairs = nullptr; void* d_refit_root = nullptr;
    void* d_stage_vtx = nullptr; void* d_stage_nrm = nullptr;
    bool refit_ready = false;                      // the device tables are there
    bool refitted = false;                         // an update has run since the upload: d_refit_root holds the root's box
    // prt_rebuild_bvh (pt_build.hip).  n_slots: the slots of the current tree (the host tables above are the UPLOADED tree's: a rebuild empties
    // slot_vtx, level_pairs and node_box -- its tables exist on the device only -- and replaces level_first); rebuilt: the tree is a rebuilt
    // one (node 0 the root, the children of pair k nodes 2k + 1 and 2k + 2).  up_nodes / up_prims: the caller's tree as uploaded, for
    // prt_read_bvh.  A rebuild writes into the `spare` set of buffers and swaps it with the live one at its end; cap_*: what the live buffers
    // hold.  d_build: the build's scratch (BuildWork bw over build_T triangles).  Spare set and scratch are allocated by the first rebuild and
    // OUTLIVE the scene: prt_upload_scene frees the live set (and with it the refit tables, the staging buffers, the snapshot and the primitive
    // tables below) but keeps the spare set and the scratch for the next scene's rebuilds -- prt_destroy alone frees them.  Nothing in them is
    // read before it is written: a rebuild sizes the spare set by spare.cap_* (grown when the new T needs more, kept when it needs less), the
    // scratch by build_T (laid out again whenever T differs), and the live capacities cap_* are set by every upload to what it allocated
    // (tests/test_call_sequences.py: uploads of fewer and of more triangles between rebuilds)
    size_t n_slots = 0;
    bool rebuilt = false;
    std::vector<prt_bvh_node> up_nodes;
    std::vector<uint64_t> up_prims;
    struct TreeSet { void* pairs = nullptr; void* tri_geom = nullptr; void* tri_nrm = nullptr; void* slot_vtx = nullptr; void* level_pairs = nullptr;
                     void* root = nullptr; void* tri_prev = nullptr; size_t cap_pairs = 0, cap_slots = 0, cap_prev = 0; } spare;
    size_t cap_pairs = 0, cap_slots = 0, cap_prev = 0;
    void* d_build = nullptr;
    uint32_t build_T = 0;
    BuildWork bw{};
    // prt_set_motion: d_tri_prev the triangle records (48 bytes per slot) as they were before the first update since the last guide render
    // (allocated by that update, freed with the scene and when motion is turned off); snap_valid: such a snapshot is pending -- the next
    // prt_render_guides consumes it.  d_motion the motion plane of the frame part (one float4 {D, m} per pixel, allocated on first use,
    // freed with the frame); motion_valid: it was written by the guide render that made guides_valid
    bool motion = false;
    void* d_tri_prev = nullptr;
    bool snap_valid = false;
    float4* d_motion = nullptr;
    bool motion_valid = false;
    // prt_update_primitives (pt_prims.hip).  mesh_t: t of every uploaded prt_mesh (host).  All of the rest is allocated by the first update and
    // freed with the scene: d_prim_types {the pack kernel's flag word, 12 bytes of padding, mesh_t}; the staging tables the pack kernel writes
    // (sized as the live ones) and d_stage_meshes, the host variant's records; with motion on, the tables as they were before the first
    // update since the last guide render (d_*_prev) -- prim_snap_valid: such a snapshot is pending, independent of the triangles' snap_valid
    std::vector<uint8_t> mesh_t;
    void* d_prim_types = nullptr;
    void* d_stage_spheres = nullptr; void* d_stage_sdfs = nullptr; void* d_stage_quads = nullptr; void* d_stage_meshes = nullptr;
    void* d_spheres_prev = nullptr; void* d_sdfs_prev = nullptr; void* d_quads_prev = nullptr;
    bool prim_snap_valid = false;
    // prt_set_smooth_normals (pt_normals.hip): the smoothing topology of the uploaded mesh on the device -- the group of every corner, the
    // group-to-members table -- and what a generation writes: the face buffer (d_sm_face_r for the area weighting only) and the generated
    // normals (float4[3T]).  All allocated by prt_set_smooth_normals, freed by turning it off, by prt_upload_scene and with the scene
    bool smooth = false;
    uint32_t smooth_weighting = 0;
    float smooth_crease = 0.0f;
    void* d_sm_group = nullptr; void* d_sm_first = nullptr; void* d_sm_member = nullptr;
    void* d_sm_face_f = nullptr; void* d_sm_face_r = nullptr; void* d_sm_nrm = nullptr;
    // prt_cast_rays / prt_occluded / prt_cast_pixels (pt_cast.hip): the host variants' staging buffers -- rays (32 bytes each; prt_cast_pixels
    // puts its (x, y) pairs behind the rays it generates) and results (48 bytes each).  Not the scene's and not the frame's: grown on demand,
    // freed by prt_destroy alone
    void* d_cast_rays = nullptr; void* d_cast_out = nullptr;
    size_t cast_rays_cap = 0, cast_out_cap = 0;
};

#define CTX_CHECK(ctx) do { if (!(ctx)) return PRT_ERR_INVALID_ARGUMENT; } while (0)
#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
        (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return PRT_ERR_HIP; } } while (0)

inline int fail(prt_ctx* ctx, int code, const std::string& msg) { ctx->err = msg; return code; }

template <typename T>
void free_dev(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

// prt_set_smooth_normals off: the topology and the generation's buffers go
inline void free_smooth(prt_ctx* c) {
    free_dev(c->d_sm_group); free_dev(c->d_sm_first); free_dev(c->d_sm_member);
    free_dev(c->d_sm_face_f); free_dev(c->d_sm_face_r); free_dev(c->d_sm_nrm);
    c->smooth = false;
}

// prt_update_primitives: the primitive snapshot (motion off, a new scene), and with `all` everything else the first update allocated
inline void free_prims(prt_ctx* c, bool all) {
    free_dev(c->d_spheres_prev); free_dev(c->d_sdfs_prev); free_dev(c->d_quads_prev);
    c->prim_snap_valid = false;
    if (!all) return;
    free_dev(c->d_prim_types); free_dev(c->d_stage_spheres); free_dev(c->d_stage_sdfs); free_dev(c->d_stage_quads); free_dev(c->d_stage_meshes);
}

// measured tile orders are the scene's, the view's and the frame's: whatever changes one of them forgets them
inline void forget_tile_orders(prt_ctx* c) { for (int j = 0; j < prt_ctx::MAX_SUB; ++j) c->have_order[j] = false; }

template <typename T>
int upload(prt_ctx* c, void*& dst, const std::vector<T>& src) {
    free_dev(dst);
    size_t bytes = (src.empty() ? 1 : src.size()) * sizeof(T);
    HIPCHK(c, hipMalloc(&dst, bytes));
    if (!src.empty()) HIPCHK(c, hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return PRT_OK;
}

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
    fa.unfinished = count ? c->d_counters : nullptr;
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
    fa.filter_tab = c->filter_kind >= PRT_FILTER_GAUSSIAN ? c->d_filter_tab : nullptr;
    return fa;
}
