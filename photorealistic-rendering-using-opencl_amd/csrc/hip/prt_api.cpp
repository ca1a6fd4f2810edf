// prt_api.cpp -- implementation of the C ABI in include/prt.h on top of HIP.
// Replaces the OpenCL host sequence of the reference's src/main.cpp (see prt.h for the
// call-by-call mapping).  No CPU fallback: every entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <string>
#include <thread>
#include <vector>
#include <algorithm>

#include "prt.h"
#include "pt_filter.h"
#include "pt_launch.h"
#include "pt_layout.h"
#include "pt_pack.h"
#include "pt_build.h"
#include "pt_refit.h"
#include "pt_variant.h"

using namespace prt;

namespace {
thread_local std::string g_global_error;
}

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
    hipEvent_t sub_ev[MAX_SUB][2] = {};           // end of a sub-part's launch (two in flight per sub-part)
    hipEvent_t sub_ev0[MAX_SUB][2] = {};          // its start (prt_render_spp times every launch)
    hipEvent_t fork_ev = nullptr;
    unsigned long long* h_unfinished = nullptr;   // pinned, [MAX_SUB][2]: written by the last wave of a launch
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
    bool test_drop_report = false;                 // option "test_drop_report" (tests only): the launches of prt_render_spp report into a spare word
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
    // prt_denoise_temporal (pt_temporal.hip): the history, allocated on first use with the frame's size, freed with the frame.  d_hist holds
    // two halves of {c, n} and {m1, m2, v, 0} planes (half hist_cur is the last call's, the other one is written by the next call: a flip of
    // hist_cur swaps them), d_hist_guides the guides of the last call; hist_cam its camera
    float4* d_hist = nullptr;
    float4* d_hist_guides = nullptr;
    int hist_cur = 0;
    bool hist_valid = false;                       // emptied by everything prt.h lists
    DevCamera hist_cam{};
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
    // prt_denoise_records_temporal: the record history (laid out as d_hist / d_hist_guides) of a rec_hist_w x rec_hist_h frame, allocated on
    // first use and with every new size, emptied by prt_reset_records_history, freed by prt_destroy
    float4* d_rec_hist = nullptr;
    float4* d_rec_hist_guides = nullptr;
    int rec_hist_w = 0, rec_hist_h = 0, rec_hist_cur = 0;
    bool rec_hist_valid = false;
    DevCamera rec_hist_cam{};
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
    // freed with the scene
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
};

#define CTX_CHECK(ctx) do { if (!(ctx)) return PRT_ERR_INVALID_ARGUMENT; } while (0)
#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
        (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return PRT_ERR_HIP; } } while (0)

static int fail(prt_ctx* ctx, int code, const std::string& msg) { ctx->err = msg; return code; }
static FrameArgs frame_args(prt_ctx* c, uint32_t first_frame, uint32_t n, const int32_t* d_seeds, uint32_t spp, bool count);

static void free_dev(void*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

extern "C" const char* prt_last_global_error(void) { return g_global_error.c_str(); }
extern "C" const char* prt_last_error(prt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_global_error.c_str(); }

extern "C" int prt_create(int device, const prt_config* cfg, prt_ctx** out) {
    if (!cfg || !out) { g_global_error = "prt_create: null argument"; return PRT_ERR_INVALID_ARGUMENT; }
    if (cfg->abi_version != PRT_ABI_VERSION) { g_global_error = "prt_create: abi_version mismatch"; return PRT_ERR_INVALID_ARGUMENT; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_global_error = std::string("prt_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count 0") + "); libprt has no CPU fallback";
        return PRT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) { g_global_error = "prt_create: device ordinal out of range"; return PRT_ERR_INVALID_ARGUMENT; }
    if (cfg->light_count > PRT_MAX_LIGHTS) { g_global_error = "prt_create: too many lights"; return PRT_ERR_INVALID_ARGUMENT; }
    if (cfg->marching_steps < 0 || cfg->marching_steps > 65536 || cfg->shadow_marching_steps < 0 || cfg->shadow_marching_steps > 65536) {
        g_global_error = "prt_create: MARCHING_STEPS / SHADOW_MARCHING_STEPS outside 0..65536 (they bound a loop every lane runs)";
        return PRT_ERR_INVALID_ARGUMENT;
    }
    if (cfg->geom_flags & PRT_GEOM_BOX) {
        g_global_error = "prt_create: box primitives never render in the reference (geometry/box.cl is not included, SURVEY.md s9-Q10)";
        return PRT_ERR_UNSUPPORTED;
    }
    prt_ctx* c = new prt_ctx();
    c->device = device;
    c->cfg = *cfg;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess ||
        (e = hipMalloc(reinterpret_cast<void**>(&c->d_counters), (4 + 2 * prt_ctx::MAX_SUB) * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemset(c->d_counters, 0, (4 + 2 * prt_ctx::MAX_SUB) * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&c->h_unfinished), (2 * prt_ctx::MAX_SUB + 1) * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming)) != hipSuccess) {
        g_global_error = std::string("prt_create: ") + hipGetErrorString(e);
        prt_destroy(c);
        return PRT_ERR_HIP;
    }
    if (const char* ev = std::getenv("PRT_STREAMS")) { const int k = std::atoi(ev); if (k >= 1 && k <= prt_ctx::MAX_SUB) { c->n_sub = k; c->n_sub_forced = true; } }
    for (int j = 0; j < c->n_sub && c->n_sub > 1; ++j)
        if ((e = hipStreamCreateWithFlags(&c->sub_stream[j], hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreate(&c->sub_ev[j][0])) != hipSuccess || (e = hipEventCreate(&c->sub_ev0[j][0])) != hipSuccess ||
            (e = hipEventCreate(&c->sub_ev[j][1])) != hipSuccess || (e = hipEventCreate(&c->sub_ev0[j][1])) != hipSuccess) {
            g_global_error = std::string("prt_create: ") + hipGetErrorString(e);
            prt_destroy(c);
            return PRT_ERR_HIP;
        }
    c->stream = c->own_stream;
    if (const char* ev = std::getenv("PRT_FRAMES_PER_LAUNCH")) { const int k = std::atoi(ev); if (k >= 1) c->frames_per_launch = (unsigned)k; }
    if (const char* ev = std::getenv("PRT_RUN_AHEAD")) c->run_ahead = std::atoi(ev) != 0 ? 1u : 0u;
    if (const char* ev = std::getenv("PRT_PACE")) c->pace = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("PRT_WALK_MIN_LANES")) { const int k = std::atoi(ev); if (k >= 1 && k <= 64) c->walk_min_lanes = (uint32_t)k; }
    if (const char* ev = std::getenv("PRT_WAVES")) { const int k = std::atoi(ev); if (k == 5 || k == 6) c->lo.waves = k; }
    if (const char* ev = std::getenv("PRT_SCATTER")) { const int k = std::atoi(ev); if (k == 0 || k == 1) c->lo.scatter = k; }
    if (const char* ev = std::getenv("PRT_GENERIC")) c->lo.generic = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("PRT_ANY_DIST")) c->lo.any_dist = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("PRT_PIX_PER_WAVE")) { const int k = std::atoi(ev); if (k == 64 || k == 32 || k == 16) c->lo.pix_per_wave = k; }
    if (const char* ev = std::getenv("PRT_POOL")) c->lo.pool = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("PRT_TRI_Q")) { const int k = std::atoi(ev); if (k >= 0 && k <= 16) c->tri_sixteenths = (uint32_t)k; }
    if (const char* ev = std::getenv("PRT_TILE_ORDER")) c->tile_sort = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("PRT_LAUNCH_LOG")) c->launch_log = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("PRT_SHADOW_MIN_LANES")) { const int k = std::atoi(ev); if (k >= 1 && k <= 64) c->shadow_min_lanes = (uint32_t)k; }
    *out = c;
    return PRT_OK;
}

static void free_frame(prt_ctx* c) {
    void* p;
    p = c->S.q0; free_dev(p); c->S.q0 = nullptr;
    p = c->S.q1; free_dev(p); c->S.q1 = nullptr;
    p = c->S.q2; free_dev(p); c->S.q2 = nullptr;
    p = c->S.q3; free_dev(p); c->S.q3 = nullptr;
    p = c->S.q4; free_dev(p); c->S.q4 = nullptr;
    p = c->fb; free_dev(p); c->fb = nullptr;
    p = c->d_adapt; free_dev(p); c->d_adapt = nullptr;
    p = c->d_live; free_dev(p); c->d_live = nullptr;
    p = c->d_live_aux; free_dev(p); c->d_live_aux = nullptr;
    p = c->d_guides; free_dev(p); c->d_guides = nullptr;
    p = c->d_dn; free_dev(p); c->d_dn = nullptr;
    p = c->d_dn_g; free_dev(p); c->d_dn_g = nullptr;
    p = c->d_hist; free_dev(p); c->d_hist = nullptr;
    p = c->d_hist_guides; free_dev(p); c->d_hist_guides = nullptr;
    p = c->d_motion; free_dev(p); c->d_motion = nullptr;
    c->motion_valid = false;
    c->guides_valid = false;
    c->hist_valid = false;
    for (int j = 0; j < prt_ctx::MAX_SUB; ++j) {
        p = c->d_tile_order[j]; free_dev(p); c->d_tile_order[j] = nullptr;
        p = c->d_tile_cost[j]; free_dev(p); c->d_tile_cost[j] = nullptr;
        c->have_order[j] = false;
    }
}
static void free_scene(prt_ctx* c) {
    free_dev(c->d_pairs); free_dev(c->d_tri_geom); free_dev(c->d_tri_nrm);
    free_dev(c->d_spheres); free_dev(c->d_quads); free_dev(c->d_sdfs); free_dev(c->d_mats); free_dev(c->d_light_tab);
    free_dev(c->d_slot_vtx); free_dev(c->d_level_pairs); free_dev(c->d_refit_root); free_dev(c->d_stage_vtx); free_dev(c->d_stage_nrm);
    c->refit_ready = c->refitted = false;
    free_dev(c->d_tri_prev);
    c->snap_valid = false;
    free_dev(c->spare.pairs); free_dev(c->spare.tri_geom); free_dev(c->spare.tri_nrm); free_dev(c->spare.slot_vtx); free_dev(c->spare.level_pairs);
    free_dev(c->spare.root); free_dev(c->spare.tri_prev); free_dev(c->d_build);
    c->spare = prt_ctx::TreeSet{};
    c->build_T = 0;
    c->cap_pairs = c->cap_slots = c->cap_prev = 0;
    c->rebuilt = false;
}

extern "C" void prt_destroy(prt_ctx* c) {
#ifdef PT_PHASE_CLOCKS
    if (c) { (void)hipDeviceSynchronize(); prt::dump_phase_clocks(); }
#endif
#ifdef PT_POOL_STATS
    if (c) { (void)hipDeviceSynchronize(); prt::dump_pool_stats(); }
#endif
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int j = 0; j < prt_ctx::MAX_SUB; ++j) {
        if (c->sub_stream[j]) { (void)hipStreamSynchronize(c->sub_stream[j]); (void)hipStreamDestroy(c->sub_stream[j]); }
        for (int k = 0; k < 2; ++k) {
            if (c->sub_ev[j][k]) (void)hipEventDestroy(c->sub_ev[j][k]);
            if (c->sub_ev0[j][k]) (void)hipEventDestroy(c->sub_ev0[j][k]);
        }
    }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->h_unfinished) (void)hipHostFree(c->h_unfinished);
    free_frame(c);
    free_scene(c);
    free_dev(c->d_env); free_dev(c->d_env_rows); free_dev(c->d_env_cols);
    void* p = c->d_seeds; free_dev(p);
    p = c->d_counters; free_dev(p);
    p = c->d_filter_tab; free_dev(p);
    p = c->d_rec; free_dev(p);
    p = c->d_rec_hist; free_dev(p);
    p = c->d_rec_hist_guides; free_dev(p);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

template <typename T>
static int upload(prt_ctx* c, void*& dst, const std::vector<T>& src) {
    free_dev(dst);
    size_t bytes = (src.empty() ? 1 : src.size()) * sizeof(T);
    HIPCHK(c, hipMalloc(&dst, bytes));
    if (!src.empty()) HIPCHK(c, hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return PRT_OK;
}

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
    c->hist_valid = false;
    // (the refit tables and staging buffers are the old tree's: a static scene holds none on the device)
    free_dev(c->d_slot_vtx); free_dev(c->d_level_pairs); free_dev(c->d_refit_root); free_dev(c->d_stage_vtx); free_dev(c->d_stage_nrm);
    c->refit_ready = c->refitted = false;
    free_dev(c->d_tri_prev);                         // (the snapshot is the old scene's: no motion across an upload)
    c->snap_valid = false;
    c->cap_prev = 0;
    c->rebuilt = false;
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
    for (int j = 0; j < prt_ctx::MAX_SUB; ++j) c->have_order[j] = false;
    return PRT_OK;
}

// ---- deforming geometry: new vertices into the uploaded tree (prt.h prt_update_vertices; pt_refit.hip) ----------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int refit_tables(prt_ctx* c);

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
static int refit_tables(prt_ctx* c) {
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
    for (int j = 0; j < prt_ctx::MAX_SUB; ++j) c->have_order[j] = false;
    c->refitted = true;
    launch_refit(t, v, n, static_cast<NodePair*>(c->d_pairs), static_cast<TriGeom*>(c->d_tri_geom), static_cast<TriNrm*>(c->d_tri_nrm),
                 static_cast<float*>(c->d_refit_root), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the caller's buffers may be reused on return
    return PRT_OK;
}

extern "C" int prt_update_vertices(prt_ctx* c, const float* vertices, const float* normals) {
    CTX_CHECK(c);
    int rc = refit_prepare(c, vertices, "prt_update_vertices");
    if (rc) return rc;
    const size_t bytes = 3 * (size_t)c->n_tris * 16;
    if (!c->d_stage_vtx) HIPCHK(c, hipMalloc(&c->d_stage_vtx, bytes));
    if (normals && !c->d_stage_nrm) HIPCHK(c, hipMalloc(&c->d_stage_nrm, bytes));
    HIPCHK(c, hipMemcpyAsync(c->d_stage_vtx, vertices, bytes, hipMemcpyHostToDevice, c->stream));
    if (normals) HIPCHK(c, hipMemcpyAsync(c->d_stage_nrm, normals, bytes, hipMemcpyHostToDevice, c->stream));
    return prt_update_vertices_device(c, c->d_stage_vtx, normals ? c->d_stage_nrm : nullptr);
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
extern "C" int prt_rebuild_bvh_device(prt_ctx* c, const void* d_vertices, const void* d_normals, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (!c->have_scene || c->n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_rebuild_bvh: no scene with triangles uploaded");
    if (!d_vertices) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: null vertices");
    if (max_leaf > 64u) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: max_leaf above 64 (the scene is unchanged)");
    if (!aligned16(d_vertices) || !aligned16(d_normals))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh_device: the device buffers must be 16-byte aligned");
    if (!max_leaf) max_leaf = PT_BUILD_DEFAULT_LEAF;
    const uint32_t T = c->n_tris;
    const bool leaf_root = T <= max_leaf;
    const bool carry_nrm = d_normals == nullptr;
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
    for (int j = 0; j < prt_ctx::MAX_SUB; ++j) c->have_order[j] = false;
    return PRT_OK;
}

extern "C" int prt_rebuild_bvh(prt_ctx* c, const float* vertices, const float* normals, uint32_t max_leaf) {
    CTX_CHECK(c);
    if (!c->have_scene || c->n_tris == 0) return fail(c, PRT_ERR_NOT_READY, "prt_rebuild_bvh: no scene with triangles uploaded");
    if (!vertices) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: null vertices");
    if (max_leaf > 64u) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_rebuild_bvh: max_leaf above 64 (the scene is unchanged)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = 3 * (size_t)c->n_tris * 16;
    if (!c->d_stage_vtx) HIPCHK(c, hipMalloc(&c->d_stage_vtx, bytes));
    if (normals && !c->d_stage_nrm) HIPCHK(c, hipMalloc(&c->d_stage_nrm, bytes));
    HIPCHK(c, hipMemcpyAsync(c->d_stage_vtx, vertices, bytes, hipMemcpyHostToDevice, c->stream));
    if (normals) HIPCHK(c, hipMemcpyAsync(c->d_stage_nrm, normals, bytes, hipMemcpyHostToDevice, c->stream));
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

extern "C" int prt_set_camera(prt_ctx* c, const prt_camera* cam) {
    CTX_CHECK(c);
    if (!cam) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_camera: null camera");
    make_dev_camera(*cam, c->cam);
    c->have_cam = true;
    c->guides_valid = false;
    for (int j = 0; j < prt_ctx::MAX_SUB; ++j) c->have_order[j] = false;      // (tile costs are the view's)
    return PRT_OK;
}

extern "C" int prt_upload_envmap(prt_ctx* c, const float* rgb, int w, int h) {
    CTX_CHECK(c);
    if (!rgb || w <= 0 || h <= 0) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_upload_envmap: bad arguments");
    if ((uint64_t)w * (uint64_t)h > PRT_MAX_ENV_TEXELS)       // (env_texel reads the map by a 32-bit byte offset, like the scene's tables)
        return fail(c, PRT_ERR_UNSUPPORTED, "prt_upload_envmap: more than 357913941 texels (PRT_MAX_ENV_TEXELS: 12-byte texels below 4 GiB, 32-bit offsets)");
    if (w > PRT_MAX_ENV_SIDE || h > PRT_MAX_ENV_SIDE)
        return fail(c, PRT_ERR_UNSUPPORTED, "prt_upload_envmap: a side of more than 16777215 texels (PRT_MAX_ENV_SIDE: the texel index is a 24-bit multiply)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->guides_valid = false;
    c->hist_valid = false;
    free_dev(c->d_env);
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    HIPCHK(c, hipMalloc(&c->d_env, bytes));
    HIPCHK(c, hipMemcpy(c->d_env, rgb, bytes, hipMemcpyHostToDevice));
    c->sc.env = static_cast<const float*>(c->d_env);
    c->sc.env_w = w; c->sc.env_h = h;
    free_dev(c->d_env_rows); free_dev(c->d_env_cols);
    c->sc.env_cdf_rows = c->sc.env_cdf_cols = nullptr;
    if (c->cfg.env_importance_sampling) {                       // the map's sampling density (pt_kernels.hip build_env_cdf)
        std::vector<float> rows, cols;
        build_env_cdf(rgb, w, h, rows, cols);
        int rc = upload(c, c->d_env_rows, rows);
        if (!rc) rc = upload(c, c->d_env_cols, cols);
        if (rc) return rc;
        c->sc.env_cdf_rows = static_cast<const float*>(c->d_env_rows);
        c->sc.env_cdf_cols = static_cast<const float*>(c->d_env_cols);
    }
    return PRT_OK;
}

static int alloc_frame(prt_ctx* c, int width, int full_height, int row0, int rows);

extern "C" int prt_set_tile(prt_ctx* c, int width, int full_height, int row0, int rows) {
    CTX_CHECK(c);
    if (width <= 0 || full_height <= 0 || rows <= 0 || row0 < 0 || row0 + rows > full_height)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_tile: bad tile");
    c->block_rows = 1; c->n_parts = 1; c->part = 0;
    return alloc_frame(c, width, full_height, row0, rows);
}

extern "C" int prt_set_row_blocks(prt_ctx* c, int width, int full_height, int block_rows, int n_parts, int part) {
    CTX_CHECK(c);
    if (width <= 0 || full_height <= 0 || block_rows <= 0 || n_parts <= 0 || part < 0 || part >= n_parts)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_row_blocks: bad arguments");
    int rows = 0;
    for (int r = 0; r < full_height; ++r) rows += ((r / block_rows) % n_parts == part);
    if (rows == 0) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_row_blocks: this part owns no rows");
    c->block_rows = block_rows; c->n_parts = n_parts; c->part = part;
    return alloc_frame(c, width, full_height, 0, rows);
}

static int alloc_frame(prt_ctx* c, int width, int full_height, int row0, int rows) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the context has no frame until every plane of the new one exists: a failed (re)allocation must leave it NOT READY,
    // never "ready" with null planes
    c->have_size = false;
    free_frame(c);
    c->npix = 0;
    const size_t npix = (size_t)width * (size_t)rows;
    hipError_t e = hipSuccess;
    void** planes[6] = {reinterpret_cast<void**>(&c->S.q0), reinterpret_cast<void**>(&c->S.q1), reinterpret_cast<void**>(&c->S.q2),
                        reinterpret_cast<void**>(&c->S.q3), reinterpret_cast<void**>(&c->S.q4), reinterpret_cast<void**>(&c->fb)};
    for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipMalloc(planes[k], npix * 16);
    const size_t n_tiles_alloc = (size_t)render_tile_count(width, rows);
    for (int j = 0; j < c->n_sub && c->n_sub > 1 && e == hipSuccess; ++j) {
        e = hipMalloc(reinterpret_cast<void**>(&c->d_tile_order[j]), n_tiles_alloc * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->d_tile_cost[j]), n_tiles_alloc * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(c->d_tile_cost[j], 0, n_tiles_alloc * sizeof(uint32_t));    // (a forced 5-wave build reports no costs: all equal then)
    }
    if (e != hipSuccess) {
        free_frame(c);
        (void)hipGetLastError();
        c->err = std::string("prt frame allocation (") + std::to_string(width) + " x " + std::to_string(rows) + "): " + hipGetErrorString(e);
        return PRT_ERR_HIP;
    }
    c->width = width; c->full_height = full_height; c->row0 = row0; c->rows = rows;
    c->npix = npix;
    c->have_size = true;
    return prt_reset(c);
}

extern "C" int prt_resize(prt_ctx* c, int width, int height) { return prt_set_tile(c, width, height, 0, height); }

extern "C" int prt_reset(prt_ctx* c) {
    CTX_CHECK(c);
    if (!c->have_size) return fail(c, PRT_ERR_NOT_READY, "prt_reset: no frame size set");
    HIPCHK(c, hipSetDevice(c->device));
    c->state_undefined = false;
    // enqueueFillBuffer(cl_flattenI, 0, ...), src/main.cpp:288
    HIPCHK(c, hipMemsetAsync(c->S.q0, 0, c->npix * 16, c->stream));
    HIPCHK(c, hipMemsetAsync(c->S.q1, 0, c->npix * 16, c->stream));
    HIPCHK(c, hipMemsetAsync(c->S.q2, 0, c->npix * 16, c->stream));
    HIPCHK(c, hipMemsetAsync(c->S.q3, 0, c->npix * 16, c->stream));
    HIPCHK(c, hipMemsetAsync(c->S.q4, 0, c->npix * 16, c->stream));
    HIPCHK(c, hipMemsetAsync(c->fb, 0, c->npix * 16, c->stream));
    if (c->d_adapt) HIPCHK(c, hipMemsetAsync(c->d_adapt, 0, c->npix * sizeof(float2), c->stream));
    c->fresh = true;
    c->stats_valid = false;
    return PRT_OK;
}

static int ensure_seeds(prt_ctx* c, const int32_t* seed_pairs, size_t n_frames) {
    if (c->seeds_cap < n_frames) {
        void* p = c->d_seeds; free_dev(p); c->d_seeds = nullptr; c->seeds_cap = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_seeds), n_frames * 2 * sizeof(int32_t)));
        c->seeds_cap = n_frames;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_seeds, seed_pairs, n_frames * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // caller may free seed_pairs on return
    return PRT_OK;
}

static int ready(prt_ctx* c, const char* who) {
    if (c->state_undefined) return fail(c, PRT_ERR_NOT_READY, std::string(who) + ": an earlier render call failed half-way; prt_reset or prt_write_state first");
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, std::string(who) + ": no scene uploaded");
    if (!c->have_cam) return fail(c, PRT_ERR_NOT_READY, std::string(who) + ": no camera set");
    if (!c->have_size) return fail(c, PRT_ERR_NOT_READY, std::string(who) + ": no frame size set");
    return PRT_OK;
}

static FrameArgs frame_args(prt_ctx* c, uint32_t first_frame, uint32_t n, const int32_t* d_seeds, uint32_t spp, bool count) {
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

// 1 / (mean path length of the frame so far) = paths started / segments executed over all pixels (one small reduction over the state planes on
// `stream`, which must be idle); 0 if nothing has been rendered yet
static float inverse_mean_path_length(prt_ctx* c, uint32_t spp, hipStream_t stream) {
    unsigned long long h[3] = {0, 0, 0};
    if (hipMemsetAsync(c->d_counters + 1, 0, 3 * sizeof(unsigned long long), stream) != hipSuccess) return 0.0f;
    launch_count(c->S, c->npix, spp, c->d_counters + 1, stream);
    if (hipMemcpyAsync(h, c->d_counters + 1, sizeof(h), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return 0.0f;
    // (the reference IS the mean: 0.9 / 1.15 / 1.3 / 1.5 / 2 x the mean were all slower)
    return (h[0] && h[1]) ? (float)((double)h[0] / (double)h[1]) : 0.0f;
}

// sub-parts the megakernel renders this frame part in (1 = one launch covers every tile)
// Sets of tiles rendered side by side on internal streams: 2 (PRT_STREAMS) -- but ONE launch for a SHORT render of a frame whose waves all
// fit on the chip at once (up to 5 120 tiles = one round at 5 waves per SIMD; `frames` = the frames the render is expected to take, at
// most two launches' worth): two half-size launches share the chip unevenly there and the render lasts as long as the slower one (512x512 x
// 64 spp: 19 ... 22 ms beside 21 ... 25 ms; one launch +5 ... 8 %, also at 128 spp; 640x640 and up: two are better or equal).  A LONG render
// of such a frame -- one rank's share of a 1080p frame at 1 024 spp, 16 launches -- wants the two sets: each covers the ends of the
// other's launches (0.375 s against 0.426 s).
static int sub_parts(const prt_ctx* c, unsigned long long frames) {
    if (!(c->n_sub > 1 && c->sub_stream[0])) return 1;
    const unsigned step = c->frames_per_launch ? c->frames_per_launch : (c->sc.n_pairs > 65536u ? 4096u : 512u);
    if (!c->n_sub_forced && render_tile_count(c->width, c->rows) <= 5120u && frames <= 2ull * step) return 1;
    return c->n_sub;
}
// the internal streams start behind everything already queued on the caller's stream ...
static int fork_streams(prt_ctx* c, int K) {
    HIPCHK(c, hipEventRecord(c->fork_ev, c->stream));
    for (int j = 0; j < K; ++j) HIPCHK(c, hipStreamWaitEvent(c->sub_stream[j], c->fork_ev, 0));
    return PRT_OK;
}
// ... and the caller's stream continues behind them
static int join_streams(prt_ctx* c, int K) {
    for (int j = 0; j < K; ++j) {
        HIPCHK(c, hipEventRecord(c->sub_ev[j][0], c->sub_stream[j]));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->sub_ev[j][0], 0));
    }
    return PRT_OK;
}

extern "C" int prt_render_frames(prt_ctx* c, uint32_t first_frame, uint32_t n_frames, const int32_t* seed_pairs) {
    CTX_CHECK(c);
    int rc = ready(c, "prt_render_frames");
    if (rc) return rc;
    if (first_frame == 0 || (n_frames && !seed_pairs)) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_frames: frames start at 1 and need seed pairs");
    HIPCHK(c, hipSetDevice(c->device));
    c->stats.launches = 0; c->stats.frames = 0; c->stats.kernel_ms = 0.0; c->stats.kernel_sum_ms = 0.0; c->stats.concurrent = 1;
    if (!n_frames) return PRT_OK;
    c->fresh = false;
    c->stats_valid = false;
    if ((rc = ensure_seeds(c, seed_pairs, n_frames))) return rc;
    const unsigned step = c->frames_per_launch ? c->frames_per_launch : (c->sc.n_pairs > 65536u ? 4096u : 512u);
    const int K = sub_parts(c, n_frames);
    c->stats.concurrent = (uint32_t)K;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (K > 1 && (rc = fork_streams(c, K))) return rc;
    for (uint32_t f = 0; f < n_frames; f += step) {
        const uint32_t n = (n_frames - f < step) ? n_frames - f : step;
        for (int j = 0; j < K; ++j) {
            FrameArgs fa = frame_args(c, first_frame + f, n, c->d_seeds + 2 * (size_t)f, 0, false);
            fa.tile_first = (uint32_t)j; fa.tile_stride = (uint32_t)K;
            c->last = launch_render(c->sc, c->cam, c->S, fa, c->fb, K > 1 ? c->sub_stream[j] : c->stream, c->lo);
            ++c->stats.launches;
        }
    }
    HIPCHK(c, hipGetLastError());
    if (K > 1 && (rc = join_streams(c, K))) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->timing_pending = true;
    c->stats.frames = n_frames;
    return PRT_OK;
}

extern "C" int prt_render_spp(prt_ctx* c, uint32_t spp, uint32_t max_frames, const int32_t* seed_pairs, uint32_t* frames_used) {
    CTX_CHECK(c);
    int rc = ready(c, "prt_render_spp");
    if (rc) return rc;
    if (!spp || !max_frames || !seed_pairs) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_spp: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    c->stats.launches = 0; c->stats.frames = 0; c->stats.kernel_ms = 0.0; c->stats.kernel_sum_ms = 0.0; c->stats.concurrent = 1;
    if ((rc = ensure_seeds(c, seed_pairs, max_frames))) return rc;
    c->fresh = false;
    c->stats_valid = false;
    const unsigned step = c->frames_per_launch ? c->frames_per_launch : (c->sc.n_pairs > 65536u ? 4096u : 512u);
    const int K = sub_parts(c, 8ull * spp);            // (a path takes 4.4 ... 7.2 segments on the BASELINE scenes)
    c->stats.concurrent = (uint32_t)K;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    uint32_t f = 0;
    unsigned long long unfinished = 1;
    float pace_inv_ref = 0.0f;                     // 1 / (the frame's mean path length): known once the first launch has retired
    // (through a big tree the launches are 4 096 frames and a render is a handful of them: 871 k triangles, 3840x2160 x 2 048 spp 4.35 without, 4.31 with)
    const bool pacing = c->pace && c->run_ahead && c->sc.n_pairs <= 65536u;
    if (K == 1) {
        while (f < max_frames && unfinished) {
            const uint32_t n = (max_frames - f < step) ? max_frames - f : step;
            HIPCHK(c, hipMemsetAsync(c->d_counters, 0, sizeof(unsigned long long), c->stream));
            FrameArgs fa = frame_args(c, 1 + f, n, c->d_seeds + 2 * (size_t)f, spp, true);
            fa.seed_frames = max_frames - f; fa.run_ahead = c->run_ahead;
            fa.pace_inv_ref = pacing ? pace_inv_ref : 0.0f;
            c->last = launch_render(c->sc, c->cam, c->S, fa, c->fb, c->stream, c->lo);
            ++c->stats.launches;
            f += n;
            HIPCHK(c, hipMemcpyAsync(&unfinished, c->d_counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (pacing && pace_inv_ref == 0.0f && unfinished) pace_inv_ref = inverse_mean_path_length(c, spp, c->stream);
        }
    } else {
        // Every sub-part advances on its own stream until its own pixels are frozen.  The last wave of a launch writes
        // the number of pixels still running to pinned host memory and clears the device counters, so there is no copy
        // or fill kernel between launches (with the other stream's kernel filling the chip those waited ~1.7 ms for a
        // wave slot) and the HIP events around a launch time the kernel alone.  A launch queued behind one that
        // reported 0 (PRT_QUEUE_DEPTH=2) finds every pixel frozen and returns at once.
        // the sub-part counters are {unfinished, waves done}; a launch that ended abnormally in an earlier call would
        // have left them non-zero and every later ticket wrong: start from zero, ordered before the fork
        HIPCHK(c, hipMemsetAsync(c->d_counters + 4, 0, 2 * prt_ctx::MAX_SUB * sizeof(unsigned long long), c->stream));
        if ((rc = fork_streams(c, K))) return rc;
        // any failure below leaves through abort_streams: kernels may still be running on the internal streams, the
        // caller's stream must not run ahead of them and the context must stay usable
        auto abort_streams = [&](int code, const std::string& msg) {
            for (int j = 0; j < K; ++j) (void)hipStreamSynchronize(c->sub_stream[j]);
            (void)hipMemsetAsync(c->d_counters + 4, 0, 2 * prt_ctx::MAX_SUB * sizeof(unsigned long long), c->stream);
            (void)hipStreamSynchronize(c->stream);
            (void)hipGetLastError();
            c->state_undefined = true;
            return fail(c, code, msg);
        };
#define SUBCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return abort_streams(PRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
        uint32_t fj[prt_ctx::MAX_SUB] = {0, 0, 0, 0};            // frames queued so far
        uint32_t f_end[prt_ctx::MAX_SUB][2] = {};                 // ... up to the end of the launch in each slot
        unsigned issued[prt_ctx::MAX_SUB] = {0, 0, 0, 0}, retired[prt_ctx::MAX_SUB] = {0, 0, 0, 0};
        uint32_t f_done[prt_ctx::MAX_SUB] = {0, 0, 0, 0};        // frames after which the sub-part reported 0
        bool stop[prt_ctx::MAX_SUB] = {false, false, false, false};
        bool exhausted = false;
        // launches queued per sub-part: 1 (the other sub-part's kernel covers the host round trip; 2 measured the same)
        static const unsigned depth = [] { const char* e = std::getenv("PRT_QUEUE_DEPTH"); return (e && std::atoi(e) == 2) ? 2u : 1u; }();
        const unsigned n_tiles = render_tile_count(c->width, c->rows);
        for (int j = 0; j < K; ++j) stop[j] = (unsigned)j >= n_tiles;      // a sub-part without tiles has nothing to do
        for (;;) {
            bool progressed = false, busy = false;
            for (int j = 0; j < K; ++j) {
                while (!stop[j] && issued[j] - retired[j] < depth && fj[j] < max_frames) {
                    const unsigned slot = issued[j] & 1u;
                    const uint32_t n = (max_frames - fj[j] < step) ? max_frames - fj[j] : step;
                    FrameArgs fa = frame_args(c, 1 + fj[j], n, c->d_seeds + 2 * (size_t)fj[j], spp, true);
                    fa.seed_frames = max_frames - fj[j]; fa.run_ahead = c->run_ahead;
                    fa.pace_inv_ref = pacing ? pace_inv_ref : 0.0f;
                    fa.unfinished = c->d_counters + 4 + 2 * j;
                    fa.unfinished_host = c->h_unfinished + 2 * j + slot;
                    if (c->test_drop_report) fa.unfinished_host = c->h_unfinished + 2 * prt_ctx::MAX_SUB;     // (tests: the report goes astray)
                    fa.tile_first = (uint32_t)j; fa.tile_stride = (uint32_t)K;
                    if (c->tile_sort && c->d_tile_cost[j] && c->sc.n_pairs > 65536u) {
                        fa.tile_order = c->have_order[j] ? c->d_tile_order[j] : nullptr;
                        fa.tile_cost = (!c->have_order[j] && issued[j] == 0u) ? c->d_tile_cost[j] : nullptr;
                    }
                    c->h_unfinished[2 * j + slot] = ~0ull;
                    // (a tile's cost is the maximum over its waves -- atomicMax in the kernel: the measuring launch starts from zero)
                    if (fa.tile_cost) SUBCHK(hipMemsetAsync(c->d_tile_cost[j], 0, (size_t)render_tile_count(c->width, c->rows) * sizeof(uint32_t), c->sub_stream[j]));
                    SUBCHK(hipEventRecord(c->sub_ev0[j][slot], c->sub_stream[j]));
                    c->last = c->last_sub[j] = launch_render(c->sc, c->cam, c->S, fa, c->fb, c->sub_stream[j], c->lo);
                    SUBCHK(hipEventRecord(c->sub_ev[j][slot], c->sub_stream[j]));
                    ++c->stats.launches;
                    fj[j] += n;
                    f_end[j][slot] = fj[j];
                    ++issued[j];
                    progressed = true;
                }
                if (issued[j] != retired[j]) {
                    busy = true;
                    const unsigned slot = retired[j] & 1u;
                    const hipError_t q = hipEventQuery(c->sub_ev[j][slot]);
                    if (q == hipErrorNotReady) continue;
                    SUBCHK(q);
                    float ms = 0.f;
                    if (hipEventElapsedTime(&ms, c->sub_ev0[j][slot], c->sub_ev[j][slot]) == hipSuccess) c->stats.kernel_sum_ms += ms;
                    const unsigned long long left = __atomic_load_n(c->h_unfinished + 2 * j + slot, __ATOMIC_ACQUIRE);
                    if (c->launch_log) std::fprintf(stderr, "prt launch: part %d #%u %.3f ms, %llu pixels unfinished\n", j, retired[j], ms, left);
                    // the host armed the slot with ~0 before the launch; the last wave of the launch overwrites it (render_kernel).  A launch whose
                    // report never arrived must not be read as 1.8e19 unfinished pixels
                    if (left == ~0ull) return abort_streams(PRT_ERR_HIP, "prt_render_spp: a launch ended without reporting its unfinished pixels");
                    if (c->tile_sort && c->d_tile_cost[j] && c->sc.n_pairs > 65536u && !c->have_order[j] && retired[j] == 0u && !c->last_sub[j].scatter && n_tiles > (unsigned)j) {
                        // launch 0 of this sub-part is over and its stream idle: its tiles by run time, longest first, for every launch from here on
                        const unsigned grid = (n_tiles - (unsigned)j + (unsigned)K - 1u) / (unsigned)K;
                        c->h_tile_cost.resize(grid); c->h_tile_order.resize(grid);
                        SUBCHK(hipMemcpyAsync(c->h_tile_cost.data(), c->d_tile_cost[j], grid * sizeof(uint32_t), hipMemcpyDeviceToHost, c->sub_stream[j]));
                        SUBCHK(hipStreamSynchronize(c->sub_stream[j]));
                        for (unsigned k = 0; k < grid; ++k) c->h_tile_order[k] = k;
                        const uint32_t* cost = c->h_tile_cost.data();
                        std::stable_sort(c->h_tile_order.begin(), c->h_tile_order.end(), [cost](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
                        SUBCHK(hipMemcpyAsync(c->d_tile_order[j], c->h_tile_order.data(), grid * sizeof(uint32_t), hipMemcpyHostToDevice, c->sub_stream[j]));
                        SUBCHK(hipStreamSynchronize(c->sub_stream[j]));      // (the host vector is reused by the other sub-part)
                        c->have_order[j] = true;
                    }
                    // the frame's mean path length, once per render (this sub-part's stream is idle: its launch has just retired)
                    if (pacing && pace_inv_ref == 0.0f && left) pace_inv_ref = inverse_mean_path_length(c, spp, c->sub_stream[j]);
                    ++retired[j];
                    progressed = true;
                    if (!stop[j]) {
                        if (left == 0) { stop[j] = true; f_done[j] = f_end[j][slot]; }
                        else if (f_end[j][slot] >= max_frames) { stop[j] = true; f_done[j] = max_frames; exhausted = true; }
                    }
                }
            }
            if (!busy && !progressed) break;
            if (!progressed) std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
#undef SUBCHK
        for (int j = 0; j < K; ++j) fj[j] = f_done[j];
        for (int j = 0; j < K; ++j) f = fj[j] > f ? fj[j] : f;
        unfinished = exhausted ? 1 : 0;
        if ((rc = join_streams(c, K))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->timing_pending = true;
    c->stats.frames = f;
    if (frames_used) *frames_used = f;
    if (unfinished) return fail(c, PRT_ERR_NOT_READY, "prt_render_spp: max_frames reached before every pixel finished");
    return PRT_OK;
}

// prt_render_adaptive (prt.h).  Rounds of launches: a round covers the same window of frames in each of the K sub-parts, on their streams,
// and waits for all of them -- their reports plan the next round.  While many pixels are live a sub-part is prt_render_spp's interleaved set
// of tiles; once fewer than compact_below % of the frame are, the live pixels are listed in increasing order (launch_live_list) and the
// sub-parts are consecutive shares of the list, which is rebuilt once its live pixels have fallen below half of it.  Every live pixel has done
// exactly the frames of the rounds so far (plus its run-ahead lead, kept in its state), so any list of them can take the next window.
extern "C" int prt_render_adaptive(prt_ctx* c, const prt_adaptive* a, uint32_t max_frames, const int32_t* seed_pairs, uint32_t* frames_used) {
    CTX_CHECK(c);
    int rc = ready(c, "prt_render_adaptive");
    if (rc) return rc;
    if (!a || !max_frames || !seed_pairs) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_adaptive: bad arguments");
    if (a->min_spp < 2 || a->max_spp < a->min_spp) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_adaptive: needs 2 <= min_spp <= max_spp");
    if (!(a->rel_err >= 0.0f) || !(a->abs_floor >= 0.0f))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_adaptive: rel_err and abs_floor must be >= 0 (and not NaN)");
    if (max_frames >= (1u << 29))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_adaptive: max_frames must be below 2^29 (the run-ahead lead shares its word with the converged bit)");
    if (c->sc.view) return fail(c, PRT_ERR_UNSUPPORTED, "prt_render_adaptive: a debug view overwrites acc: there is no noise to judge");
    if (!c->fresh) return fail(c, PRT_ERR_NOT_READY, "prt_render_adaptive: needs a freshly reset context (prt_reset)");
    HIPCHK(c, hipSetDevice(c->device));
    c->stats.launches = 0; c->stats.frames = 0; c->stats.kernel_ms = 0.0; c->stats.kernel_sum_ms = 0.0; c->stats.concurrent = 1;
    c->arep = prt_adaptive_report{};
    if ((rc = ensure_seeds(c, seed_pairs, max_frames))) return rc;
    const unsigned n_waves = (unsigned)((c->npix + 63) / 64);
    if (!c->d_adapt) {
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_adapt), c->npix * sizeof(float2)));
        HIPCHK(c, hipMemsetAsync(c->d_adapt, 0, c->npix * sizeof(float2), c->stream));
    }
    if (!c->d_live) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_live), c->npix * sizeof(uint32_t)));
    if (!c->d_live_aux) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_live_aux), (n_waves + 1) * sizeof(uint32_t)));
    c->fresh = false;
    c->stats_valid = true;                       // (prt_denoise PRT_DENOISE_VAR_STATS)
    const unsigned step = c->frames_per_launch ? c->frames_per_launch : (c->sc.n_pairs > 65536u ? 4096u : 512u);
    const int K = sub_parts(c, 8ull * a->max_spp);
    c->stats.concurrent = (uint32_t)K;
    const bool pacing = c->pace && c->run_ahead && c->sc.n_pairs <= 65536u;
    float pace_inv_ref = 0.0f;
    const unsigned n_tiles = render_tile_count(c->width, c->rows);
    HIPCHK(c, hipMemsetAsync(c->d_counters + 4, 0, 2 * prt_ctx::MAX_SUB * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (K > 1 && (rc = fork_streams(c, K))) return rc;
    auto stream_of = [&](int j) { return K > 1 ? c->sub_stream[j] : c->stream; };
    auto abort_streams = [&](int code, const std::string& msg) {
        for (int j = 0; j < K; ++j) (void)hipStreamSynchronize(stream_of(j));
        (void)hipMemsetAsync(c->d_counters + 4, 0, 2 * prt_ctx::MAX_SUB * sizeof(unsigned long long), c->stream);
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        c->state_undefined = true;
        return fail(c, code, msg);
    };
#define SUBCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return abort_streams(PRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
    bool done[prt_ctx::MAX_SUB] = {false, false, false, false};     // tile rounds: every pixel of the sub-part's tiles is frozen
    for (int j = 0; j < K; ++j) done[j] = (unsigned)j >= n_tiles;
    unsigned long long live = c->npix;
    uint32_t list_count = 0;
    bool list_mode = false;
    uint32_t f = 0;
    while (f < max_frames && live) {
        const uint32_t n = (max_frames - f < step) ? max_frames - f : step;
        if (c->compact && live * 100ull < (unsigned long long)c->npix * (unsigned)c->compact_below && (!list_mode || 2ull * live < list_count)) {
            // (every stream is idle: the last round has been waited for)
            launch_live_list(c->S, c->npix, a->max_spp, c->d_live_aux, c->d_live, c->d_live_aux + n_waves, c->stream);
            uint32_t cnt = 0;
            SUBCHK(hipMemcpyAsync(&cnt, c->d_live_aux + n_waves, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
            SUBCHK(hipStreamSynchronize(c->stream));
            if (cnt != live) return abort_streams(PRT_ERR_HIP, "prt_render_adaptive: the live-pixel list disagrees with the launches' reports");
            list_count = cnt; list_mode = true;
            ++c->arep.list_builds;
        }
        const uint32_t chunk = list_mode ? (((list_count + 63u) / 64u + (uint32_t)K - 1u) / (uint32_t)K) * 64u : 0u;   // (whole waves per sub-part)
        bool launched[prt_ctx::MAX_SUB] = {false, false, false, false};
        for (int j = 0; j < K; ++j) {
            FrameArgs fa = frame_args(c, 1 + f, n, c->d_seeds + 2 * (size_t)f, a->max_spp, true);
            fa.seed_frames = max_frames - f; fa.run_ahead = c->run_ahead;
            fa.pace_inv_ref = pacing ? pace_inv_ref : 0.0f;
            fa.adapt = c->d_adapt; fa.min_spp = a->min_spp; fa.rel_err = a->rel_err; fa.abs_floor = a->abs_floor;
            fa.unfinished = c->d_counters + 4 + 2 * j;
            fa.unfinished_host = c->h_unfinished + 2 * j;
            if (list_mode) {
                const uint32_t start = (uint32_t)j * chunk;
                if (start >= list_count) continue;
                fa.live = c->d_live + start;
                fa.live_count = std::min(chunk, list_count - start);
                c->arep.list_lanes += 64ull * ((fa.live_count + 63u) / 64u);
                ++c->arep.list_launches;
            } else {
                if (done[j]) continue;
                fa.tile_first = (uint32_t)j; fa.tile_stride = (uint32_t)K;
                ++c->arep.tile_launches;
            }
            c->h_unfinished[2 * j] = ~0ull;
            if (K > 1) SUBCHK(hipEventRecord(c->sub_ev0[j][0], stream_of(j)));
            c->last = launch_render(c->sc, c->cam, c->S, fa, c->fb, stream_of(j), c->lo);
            if (K > 1) SUBCHK(hipEventRecord(c->sub_ev[j][0], stream_of(j)));
            ++c->stats.launches;
            launched[j] = true;
        }
        if (list_mode) c->arep.list_live_lanes += live;
        SUBCHK(hipGetLastError());
        live = 0;
        for (int j = 0; j < K; ++j) {
            if (!launched[j]) continue;
            SUBCHK(hipStreamSynchronize(stream_of(j)));
            float ms = 0.f;
            if (K > 1 && hipEventElapsedTime(&ms, c->sub_ev0[j][0], c->sub_ev[j][0]) == hipSuccess) c->stats.kernel_sum_ms += ms;
            const unsigned long long left = __atomic_load_n(c->h_unfinished + 2 * j, __ATOMIC_ACQUIRE);
            if (c->launch_log) std::fprintf(stderr, "prt adaptive launch: part %d frames %u..%u %s %.3f ms, %llu pixels unfinished\n", j, 1 + f, f + n,
                                            list_mode ? "list" : "tiles", ms, left);
            if (left == ~0ull) return abort_streams(PRT_ERR_HIP, "prt_render_adaptive: a launch ended without reporting its unfinished pixels");
            if (!list_mode) done[j] = left == 0;
            live += left;
        }
        f += n;
        if (pacing && pace_inv_ref == 0.0f && live) pace_inv_ref = inverse_mean_path_length(c, a->max_spp, c->stream);
    }
#undef SUBCHK
    if (K > 1 && (rc = join_streams(c, K))) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->timing_pending = true;
    c->stats.frames = f;
    if (frames_used) *frames_used = f;
    if (live) return fail(c, PRT_ERR_NOT_READY, "prt_render_adaptive: max_frames reached before every pixel froze");
    return PRT_OK;
}

extern "C" int prt_read_adaptive_stats(prt_ctx* c, float* out2) {
    CTX_CHECK(c);
    if (!out2 || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_adaptive_stats: bad arguments");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    if (!c->d_adapt) { std::memset(out2, 0, c->npix * 2 * sizeof(float)); return PRT_OK; }    // (no adaptive render since the frame was made)
    HIPCHK(c, hipMemcpy(out2, c->d_adapt, c->npix * sizeof(float2), hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_get_adaptive_report(prt_ctx* c, prt_adaptive_report* out) {
    CTX_CHECK(c);
    if (!out) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_get_adaptive_report: null");
    *out = c->arep;
    return PRT_OK;
}

extern "C" int prt_render_guides(prt_ctx* c, uint32_t samples) {
    CTX_CHECK(c);
    int rc = ready(c, "prt_render_guides");
    if (rc) return rc;
    if (samples < 1 || samples > 64) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_guides: samples must be 1 .. 64");
    HIPCHK(c, hipSetDevice(c->device));
    c->guides_valid = false;
    c->motion_valid = false;
    if (!c->d_guides) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_guides), c->npix * 2 * sizeof(float4)));
    if (c->motion && !c->d_motion) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_motion), c->npix * sizeof(float4)));
    const bool snap = c->motion && c->snap_valid && c->d_tri_prev;
    // the motion instances only where there is a snapshot to measure from; no update since the last guide render: the plain kernels and a
    // plane of zeros
    if (snap) launch_guides_motion(c->sc, c->cam, frame_args(c, 1, 0, nullptr, 0, false), samples, c->d_guides,
                                   static_cast<const TriGeom*>(c->d_tri_prev), c->d_motion, c->stream);
    else launch_guides(c->sc, c->cam, frame_args(c, 1, 0, nullptr, 0, false), samples, c->d_guides, c->stream);
    HIPCHK(c, hipGetLastError());
    if (c->motion && !snap) HIPCHK(c, hipMemsetAsync(c->d_motion, 0, c->npix * sizeof(float4), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->guides_valid = true;
    if (c->motion) {
        c->snap_valid = false;                         // consumed: the next plane is measured from the geometry these guides saw
        c->motion_valid = true;
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
    }
    return PRT_OK;
}

static int motion_ready(prt_ctx* c, const char* who) {
    const std::string w(who);
    if (!c->motion) return fail(c, PRT_ERR_NOT_READY, w + ": motion is off (prt_set_motion)");
    if (!c->guides_valid || !c->motion_valid || !c->d_motion)
        return fail(c, PRT_ERR_NOT_READY, w + ": no guides with a motion plane for this scene, camera, map and frame (prt_render_guides)");
    return PRT_OK;
}

extern "C" int prt_read_motion(prt_ctx* c, float* out4) {
    CTX_CHECK(c);
    if (!out4 || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_motion: bad arguments");
    int rc = motion_ready(c, "prt_read_motion");
    if (rc) return rc;
    if ((rc = prt_synchronize(c))) return rc;
    HIPCHK(c, hipMemcpy(out4, c->d_motion, c->npix * sizeof(float4), hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_export_motion(prt_ctx* c, void* device_motion) {
    CTX_CHECK(c);
    if (!device_motion || !aligned16(device_motion) || !c->have_size)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_export_motion: bad arguments (a 16-byte aligned device pointer, a context with a frame size)");
    int rc = motion_ready(c, "prt_export_motion");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(device_motion, c->d_motion, c->npix * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    if (c->stream == c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));       // (as prt_export_denoise_inputs)
    return PRT_OK;
}

extern "C" int prt_read_guides(prt_ctx* c, float* out8) {
    CTX_CHECK(c);
    if (!out8 || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_guides: bad arguments");
    if (!c->guides_valid) return fail(c, PRT_ERR_NOT_READY, "prt_read_guides: no guides for this scene, camera, map and frame (prt_render_guides)");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out8, c->d_guides, c->npix * 2 * sizeof(float4), hipMemcpyDeviceToHost));
    return PRT_OK;
}

// the parameter checks of every denoise call ...
static int denoise_param_checks(prt_ctx* c, const prt_denoise_params& p, const char* who) {
    const std::string w(who);
    if (p.passes < 1 || p.passes > 8) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": passes must be 1 .. 8");
    if (!(p.sigma_l > 0.0f) || !(p.sigma_n > 0.0f) || !(p.sigma_z > 0.0f) || !(p.sigma_a > 0.0f))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": every sigma must be > 0 (and not NaN)");
    if (p.var_source > PRT_DENOISE_VAR_SPATIAL) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": unknown var_source");
    return PRT_OK;
}
// ... and of the temporal ones
static int temporal_param_checks(prt_ctx* c, const prt_temporal_params& t, const char* who) {
    const std::string w(who);
    if (!(t.alpha_color >= 0.0f && t.alpha_color <= 1.0f) || !(t.alpha_moments >= 0.0f && t.alpha_moments <= 1.0f))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": alpha_color and alpha_moments must be in [0, 1]");
    if (!(t.tau_z > 0.0f)) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": tau_z must be > 0 (and not NaN)");
    if (!(t.cos_n >= -1.0f && t.cos_n <= 1.0f)) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": cos_n must be in [-1, 1]");
    if (t.history_cap < 1) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": history_cap must be >= 1");
    if (t.feedback > PRT_TEMPORAL_FEEDBACK_ATROUS) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": unknown feedback");
    return PRT_OK;
}

// the checks prt_denoise and prt_denoise_temporal share; *spatial: the variance source the call resolves to
static int denoise_checks(prt_ctx* c, const prt_denoise_params& p, const char* who, bool* spatial) {
    const std::string w(who);
    int rc = denoise_param_checks(c, p, who);
    if (rc) return rc;
    rc = ready(c, who);
    if (rc) return rc;
    if (c->row0 != 0 || c->rows != c->full_height || c->n_parts != 1)
        return fail(c, PRT_ERR_UNSUPPORTED, w + ": the filter needs the whole frame (tile and row-block contexts are refused)");
    if (c->sc.view) return fail(c, PRT_ERR_UNSUPPORTED, w + ": a debug view is not a picture to filter");
    if (!c->guides_valid) return fail(c, PRT_ERR_NOT_READY, w + ": no guides for this scene, camera, map and frame (prt_render_guides)");
    if (c->fresh) return fail(c, PRT_ERR_NOT_READY, w + ": nothing rendered since the reset");
    const bool stats = c->stats_valid && c->d_adapt;
    if (p.var_source == PRT_DENOISE_VAR_STATS && !stats)
        return fail(c, PRT_ERR_NOT_READY, w + ": PRT_DENOISE_VAR_STATS needs the last render since the reset to be prt_render_adaptive");
    *spatial = p.var_source == PRT_DENOISE_VAR_SPATIAL || (p.var_source == PRT_DENOISE_VAR_AUTO && !stats);
    return PRT_OK;
}

// the filtered plane `out` to the caller: rgba (prt_read_framebuffer's layout) and / or rgba8 (prt_tonemap_rgba8's transform); both may be NULL
static int denoise_output(prt_ctx* c, const float4* out, float* rgba, uint8_t* rgba8) {
    if (rgba8) {
        unsigned char* d = nullptr;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), c->npix * 4));
        launch_tonemap(out, d, frame_args(c, 1, 0, nullptr, 0, false), c->stream);
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(rgba8, d, c->npix * 4, hipMemcpyDeviceToHost);
        (void)hipFree(d);
        HIPCHK(c, e);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rgba) HIPCHK(c, hipMemcpy(rgba, out, c->npix * 16, hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_denoise(prt_ctx* c, const prt_denoise_params* params, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    prt_denoise_params p{PRT_DENOISE_DEFAULT_PASSES, PRT_DENOISE_VAR_AUTO, PRT_DENOISE_DEFAULT_SIGMA_L, PRT_DENOISE_DEFAULT_SIGMA_N,
                         PRT_DENOISE_DEFAULT_SIGMA_Z, PRT_DENOISE_DEFAULT_SIGMA_A};
    if (params) p = *params;
    bool spatial = false;
    int rc = denoise_checks(c, p, "prt_denoise", &spatial);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_dn) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_dn), c->npix * 3 * sizeof(float4)));
    if (!c->d_dn_g) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_dn_g), c->npix * sizeof(float)));
    float4* out = c->d_dn + 2 * c->npix;
    launch_denoise(c->fb, c->S.q4, c->d_adapt, spatial, c->d_guides, c->width, c->rows, p, c->d_dn, c->d_dn + c->npix, c->d_dn_g, out, c->stream);
    HIPCHK(c, hipGetLastError());
    return denoise_output(c, out, rgba, rgba8);
}

extern "C" int prt_denoise_temporal(prt_ctx* c, const prt_denoise_params* spatial, const prt_temporal_params* temporal, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    prt_denoise_params p{PRT_DENOISE_DEFAULT_PASSES, PRT_DENOISE_VAR_AUTO, PRT_DENOISE_DEFAULT_SIGMA_L, PRT_DENOISE_DEFAULT_SIGMA_N,
                         PRT_DENOISE_DEFAULT_SIGMA_Z, PRT_DENOISE_DEFAULT_SIGMA_A};
    if (spatial) p = *spatial;
    prt_temporal_params t{PRT_TEMPORAL_DEFAULT_ALPHA_COLOR, PRT_TEMPORAL_DEFAULT_ALPHA_MOMENTS, PRT_TEMPORAL_DEFAULT_TAU_Z, PRT_TEMPORAL_DEFAULT_COS_N,
                          PRT_TEMPORAL_DEFAULT_HISTORY_CAP, PRT_TEMPORAL_FEEDBACK_ATROUS};
    if (temporal) t = *temporal;
    int rc = temporal_param_checks(c, t, "prt_denoise_temporal");
    if (rc) return rc;
    bool spatial_var = false;
    rc = denoise_checks(c, p, "prt_denoise_temporal", &spatial_var);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_dn) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_dn), c->npix * 3 * sizeof(float4)));
    if (!c->d_dn_g) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_dn_g), c->npix * sizeof(float)));
    if (!c->d_hist) {
        c->hist_valid = false;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_hist), c->npix * 4 * sizeof(float4)));
    }
    if (!c->d_hist_guides) {
        c->hist_valid = false;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_hist_guides), c->npix * 2 * sizeof(float4)));
    }
    float4* half_prev = c->d_hist + 2 * c->npix * (size_t)c->hist_cur;          // {c, n} plane, then {m1, m2, v, 0}
    float4* half_next = c->d_hist + 2 * c->npix * (size_t)(c->hist_cur ^ 1);
    TemporalHistory h;
    h.cn_prev = half_prev; h.m_prev = half_prev + c->npix; h.guides_prev = c->d_hist_guides; h.cam_prev = c->hist_cam; h.valid = c->hist_valid;
    h.cn = half_next; h.m = half_next + c->npix;
    float4* out = c->d_dn + 2 * c->npix;
    c->hist_valid = false;                         // (until the call has run: a failure leaves the history empty)
    // the context's motion plane when motion is on and the plane is the valid guides' own (prt.h)
    const float4* motion = (c->motion && c->motion_valid) ? c->d_motion : nullptr;
    launch_denoise_temporal(c->fb, c->S.q4, c->d_adapt, spatial_var, c->d_guides, c->width, c->rows, p, t, c->cam, h, c->d_dn,
                            c->d_dn + c->npix, c->d_dn_g, out, c->stream, motion);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->d_hist_guides, c->d_guides, c->npix * 2 * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->hist_cur ^= 1;
    c->hist_cam = c->cam;
    c->hist_valid = true;
    return denoise_output(c, out, rgba, rgba8);
}

extern "C" int prt_read_history(prt_ctx* c, float* out8) {
    CTX_CHECK(c);
    if (!out8 || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_history: bad arguments");
    if (!c->hist_valid) return fail(c, PRT_ERR_NOT_READY, "prt_read_history: the history is empty (prt_denoise_temporal)");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    std::vector<float4> h(2 * c->npix);
    HIPCHK(c, hipMemcpy(h.data(), c->d_hist + 2 * c->npix * (size_t)c->hist_cur, 2 * c->npix * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < c->npix; ++k) {
        const float4 a = h[k], b = h[c->npix + k];
        float* o = out8 + 8 * k;
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    }
    return PRT_OK;
}

extern "C" int prt_reset_history(prt_ctx* c) {
    CTX_CHECK(c);
    c->hist_valid = false;
    return PRT_OK;
}

// ---- denoiser inputs as records (prt.h prt_export_denoise_inputs, prt_denoise_records; pt_records.hip) ---------------------------------------
extern "C" int prt_export_denoise_inputs(prt_ctx* c, void* device_records) {
    CTX_CHECK(c);
    if (!device_records || !aligned16(device_records) || !c->have_size)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_export_denoise_inputs: bad arguments (a 16-byte aligned device pointer, a context with a frame size)");
    if (c->state_undefined) return fail(c, PRT_ERR_NOT_READY, "prt_export_denoise_inputs: an earlier render call failed half-way; prt_reset or prt_write_state first");
    if (c->sc.view) return fail(c, PRT_ERR_UNSUPPORTED, "prt_export_denoise_inputs: a debug view is not a picture to filter");
    if (!c->guides_valid) return fail(c, PRT_ERR_NOT_READY, "prt_export_denoise_inputs: no guides for this scene, camera, map and frame (prt_render_guides)");
    if (c->fresh) return fail(c, PRT_ERR_NOT_READY, "prt_export_denoise_inputs: nothing rendered since the reset");
    HIPCHK(c, hipSetDevice(c->device));
    const bool stats = c->stats_valid && c->d_adapt;
    launch_records_export(c->fb, c->S.q4, stats ? c->d_adapt : nullptr, c->d_guides, c->width, c->rows, static_cast<float4*>(device_records), c->stream);
    HIPCHK(c, hipGetLastError());
    // (prt_copy_framebuffer_to_device: on a caller's stream the records are ordered like the caller's other work; the context's own stream is
    // private: finish before returning)
    if (c->stream == c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// the filtered W x H plane `out` to the caller: device_rgba (device memory), rgba and rgba8 (host, as denoise_output's); any may be NULL
static int records_output(prt_ctx* c, const float4* out, int W, int H, void* device_rgba, float* rgba, uint8_t* rgba8) {
    const size_t npix = (size_t)W * (size_t)H;
    if (device_rgba) HIPCHK(c, hipMemcpyAsync(device_rgba, out, npix * 16, hipMemcpyDeviceToDevice, c->stream));
    if (rgba8) {
        FrameArgs fa = frame_args(c, 1, 0, nullptr, 0, false);
        fa.width = W; fa.full_height = H; fa.row0 = 0; fa.rows = H; fa.block_rows = 1; fa.n_parts = 1; fa.part = 0;
        unsigned char* d = nullptr;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), npix * 4));
        launch_tonemap(out, d, fa, c->stream);
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(rgba8, d, npix * 4, hipMemcpyDeviceToHost);
        (void)hipFree(d);
        HIPCHK(c, e);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rgba) HIPCHK(c, hipMemcpy(rgba, out, npix * 16, hipMemcpyDeviceToHost));
    return PRT_OK;
}

// prt_denoise_records (t, cam null) and prt_denoise_records_temporal (device_motion: null, or prt_denoise_records_temporal_motion's plane)
static int denoise_records(prt_ctx* c, const char* who, const prt_denoise_params& p, const prt_temporal_params* t, const prt_camera* cam, int W,
                           int H, const void* device_records, void* device_rgba, float* rgba, uint8_t* rgba8, const void* device_motion = nullptr) {
    const std::string w(who);
    if (W < 1 || H < 1 || !device_records || !aligned16(device_records) || (device_rgba && !aligned16(device_rgba)) || !aligned16(device_motion))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": needs width >= 1, height >= 1 and 16-byte aligned device pointers (records not null)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)W * (size_t)H;
    if (c->rec_cap < npix) {
        void* q = c->d_rec; free_dev(q); c->d_rec = nullptr; c->rec_cap = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_rec), npix * (6 * sizeof(float4) + sizeof(float)) + sizeof(unsigned)));
        c->rec_cap = npix;
    }
    float4* fb = c->d_rec;
    float4* guides = fb + npix;
    float4* buf0 = fb + 3 * npix;
    float4* buf1 = fb + 4 * npix;
    float4* out = fb + 5 * npix;
    float* g = reinterpret_cast<float*>(fb + 6 * npix);
    unsigned* d_flag = reinterpret_cast<unsigned*>(g + npix);
    float4* var = t ? buf1 : buf0;                   // (where the variance step of launch_denoise_temporal / launch_denoise leaves {rgb, v})
    HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(unsigned), c->stream));
    launch_records_import(static_cast<const float4*>(device_records), W, H, fb, guides, var, d_flag, c->stream);
    HIPCHK(c, hipGetLastError());
    bool spatial = p.var_source == PRT_DENOISE_VAR_SPATIAL;
    if (!spatial) {
        unsigned no_stats = 0;
        HIPCHK(c, hipMemcpyAsync(&no_stats, d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (no_stats && p.var_source == PRT_DENOISE_VAR_STATS)
            return fail(c, PRT_ERR_NOT_READY, w + ": PRT_DENOISE_VAR_STATS needs stats in every record (rendered by prt_render_adaptive)");
        spatial = no_stats != 0;
    }
    if (spatial) launch_denoise_var(fb, nullptr, nullptr, true, W, H, var, c->stream);       // the 5x5 moments of the gathered colours
    if (!t) {
        float4* cur = buf0;
        float4* nxt = buf1;
        for (unsigned i = 0; i < p.passes; ++i) {
            const bool last = i + 1 == p.passes;
            launch_denoise_pass(cur, guides, W, H, p, i, g, last ? fb : nullptr, last ? out : nxt, c->stream);
            float4* tmp = cur; cur = nxt; nxt = tmp;
        }
        HIPCHK(c, hipGetLastError());
        return records_output(c, out, W, H, device_rgba, rgba, rgba8);
    }
    if (!c->d_rec_hist || !c->d_rec_hist_guides || c->rec_hist_w != W || c->rec_hist_h != H) {
        c->rec_hist_valid = false;
        void* q = c->d_rec_hist; free_dev(q); c->d_rec_hist = nullptr;
        q = c->d_rec_hist_guides; free_dev(q); c->d_rec_hist_guides = nullptr;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_rec_hist), npix * 4 * sizeof(float4)));
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_rec_hist_guides), npix * 2 * sizeof(float4)));
        c->rec_hist_w = W; c->rec_hist_h = H;
    }
    DevCamera dc;
    make_dev_camera(*cam, dc);
    float4* half_prev = c->d_rec_hist + 2 * npix * (size_t)c->rec_hist_cur;
    float4* half_next = c->d_rec_hist + 2 * npix * (size_t)(c->rec_hist_cur ^ 1);
    TemporalHistory h;
    h.cn_prev = half_prev; h.m_prev = half_prev + npix; h.guides_prev = c->d_rec_hist_guides; h.cam_prev = c->rec_hist_cam; h.valid = c->rec_hist_valid;
    h.cn = half_next; h.m = half_next + npix;
    c->rec_hist_valid = false;                     // (until the call has run: a failure leaves the history empty)
    launch_denoise_temporal_var(fb, guides, W, H, p, *t, dc, h, buf0, buf1, g, out, c->stream, static_cast<const float4*>(device_motion));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->d_rec_hist_guides, guides, npix * 2 * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rec_hist_cur ^= 1;
    c->rec_hist_cam = dc;
    c->rec_hist_valid = true;
    return records_output(c, out, W, H, device_rgba, rgba, rgba8);
}

extern "C" int prt_denoise_records(prt_ctx* c, const prt_denoise_params* params, int width, int height, const void* device_records,
                                   void* device_rgba, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    prt_denoise_params p{PRT_DENOISE_DEFAULT_PASSES, PRT_DENOISE_VAR_AUTO, PRT_DENOISE_DEFAULT_SIGMA_L, PRT_DENOISE_DEFAULT_SIGMA_N,
                         PRT_DENOISE_DEFAULT_SIGMA_Z, PRT_DENOISE_DEFAULT_SIGMA_A};
    if (params) p = *params;
    int rc = denoise_param_checks(c, p, "prt_denoise_records");
    if (rc) return rc;
    return denoise_records(c, "prt_denoise_records", p, nullptr, nullptr, width, height, device_records, device_rgba, rgba, rgba8);
}

extern "C" int prt_denoise_records_temporal_motion(prt_ctx* c, const prt_denoise_params* spatial, const prt_temporal_params* temporal,
                                                   const prt_camera* cam, int width, int height, const void* device_records,
                                                   const void* device_motion, void* device_rgba, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    prt_denoise_params p{PRT_DENOISE_DEFAULT_PASSES, PRT_DENOISE_VAR_AUTO, PRT_DENOISE_DEFAULT_SIGMA_L, PRT_DENOISE_DEFAULT_SIGMA_N,
                         PRT_DENOISE_DEFAULT_SIGMA_Z, PRT_DENOISE_DEFAULT_SIGMA_A};
    if (spatial) p = *spatial;
    prt_temporal_params t{PRT_TEMPORAL_DEFAULT_ALPHA_COLOR, PRT_TEMPORAL_DEFAULT_ALPHA_MOMENTS, PRT_TEMPORAL_DEFAULT_TAU_Z, PRT_TEMPORAL_DEFAULT_COS_N,
                          PRT_TEMPORAL_DEFAULT_HISTORY_CAP, PRT_TEMPORAL_FEEDBACK_ATROUS};
    if (temporal) t = *temporal;
    const char* who = device_motion ? "prt_denoise_records_temporal_motion" : "prt_denoise_records_temporal";
    int rc = temporal_param_checks(c, t, who);
    if (!rc) rc = denoise_param_checks(c, p, who);
    if (rc) return rc;
    if (!cam) return fail(c, PRT_ERR_INVALID_ARGUMENT, std::string(who) + ": null camera");
    return denoise_records(c, who, p, &t, cam, width, height, device_records, device_rgba, rgba, rgba8, device_motion);
}

extern "C" int prt_denoise_records_temporal(prt_ctx* c, const prt_denoise_params* spatial, const prt_temporal_params* temporal, const prt_camera* cam,
                                            int width, int height, const void* device_records, void* device_rgba, float* rgba, uint8_t* rgba8) {
    return prt_denoise_records_temporal_motion(c, spatial, temporal, cam, width, height, device_records, nullptr, device_rgba, rgba, rgba8);
}

extern "C" int prt_reset_records_history(prt_ctx* c) {
    CTX_CHECK(c);
    c->rec_hist_valid = false;
    return PRT_OK;
}

extern "C" int prt_read_records_history(prt_ctx* c, int width, int height, float* out8) {
    CTX_CHECK(c);
    if (!out8 || width < 1 || height < 1) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_records_history: bad arguments");
    if (!c->rec_hist_valid || !c->d_rec_hist)
        return fail(c, PRT_ERR_NOT_READY, "prt_read_records_history: the record history is empty (prt_denoise_records_temporal)");
    if (width != c->rec_hist_w || height != c->rec_hist_h)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_records_history: the record history has another size");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    const size_t npix = (size_t)width * (size_t)height;
    std::vector<float4> h(2 * npix);
    HIPCHK(c, hipMemcpy(h.data(), c->d_rec_hist + 2 * npix * (size_t)c->rec_hist_cur, 2 * npix * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < npix; ++k) {
        const float4 a = h[k], b = h[npix + k];
        float* o = out8 + 8 * k;
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    }
    return PRT_OK;
}

// ---- the pixel filter (prt.h prt_set_pixel_filter) ------------------------------------------------------------------------------------------
static const char* const k_filter_names[] = {"none", "box", "tent", "gaussian", "blackman-harris"};

// the radius a (kind, radius) pair means: PRT_FILTER_DEFAULT_RADIUS = the kind's default; false for an unknown kind or a radius outside [0, 4]
// (NaN and the infinities included)
static bool filter_radius(uint32_t kind, float radius, float& r) {
    static const float defaults[] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f};
    if (kind > PRT_FILTER_BLACKMAN_HARRIS) return false;
    if (radius == PRT_FILTER_DEFAULT_RADIUS) { r = defaults[kind]; return true; }
    if (!(radius >= 0.0f && radius <= 4.0f)) return false;
    r = kind == PRT_FILTER_NONE ? 0.0f : radius;
    return true;
}

extern "C" int prt_set_pixel_filter(prt_ctx* c, uint32_t kind, float radius) {
    CTX_CHECK(c);
    float r = 0.0f;
    if (!filter_radius(kind, radius, r))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_pixel_filter: unknown kind, or a radius outside 0 .. 4 (PRT_FILTER_DEFAULT_RADIUS: the kind's default)");
    if (kind != PRT_FILTER_NONE) {
        const char* no = filter_unsupported(c->cfg);
        if (no) return fail(c, PRT_ERR_UNSUPPORTED, std::string("prt_set_pixel_filter: no filter instances are built for ") + no);
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));            // (launches still queued read the current table)
    if (kind >= PRT_FILTER_GAUSSIAN) {
        float tab[PT_FILTER_TAB + 1];
        build_filter_table(kind, r, tab);
        if (!c->d_filter_tab) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->d_filter_tab), sizeof(tab)));
        HIPCHK(c, hipMemcpy(c->d_filter_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
    }
    c->filter_kind = kind;
    c->filter_r = r;
    c->guides_valid = false;                               // (the temporal history is kept, as by prt_set_camera)
    return c->have_size ? prt_reset(c) : PRT_OK;
}

extern "C" int prt_pixel_filter_offsets(uint32_t kind, float radius, uint32_t gx, uint32_t gy, uint32_t k0, uint32_t n, float* out2) {
    float r = 0.0f;
    if (!filter_radius(kind, radius, r)) {
        g_global_error = "prt_pixel_filter_offsets: unknown kind, or a radius outside 0 .. 4";
        return PRT_ERR_INVALID_ARGUMENT;
    }
    if (n && !out2) { g_global_error = "prt_pixel_filter_offsets: null output"; return PRT_ERR_INVALID_ARGUMENT; }
    float tab[PT_FILTER_TAB + 1] = {};
    if (kind >= PRT_FILTER_GAUSSIAN) build_filter_table(kind, r, tab);
    for (uint32_t i = 0; i < n; ++i) {
        if (kind == PRT_FILTER_NONE) { out2[2 * i] = 0.0f; out2[2 * i + 1] = 0.0f; continue; }
        dev::filter_offset(kind, r, tab, gx, gy, k0 + i, out2[2 * i], out2[2 * i + 1]);
    }
    return PRT_OK;
}

extern "C" int prt_env_cdf(const float* rgb, int w, int h, float* rows, float* cols) {
    if (!rgb || !rows || !cols || w <= 0 || h <= 0) { g_global_error = "prt_env_cdf: bad arguments"; return PRT_ERR_INVALID_ARGUMENT; }
    std::vector<float> r, c;
    build_env_cdf(rgb, w, h, r, c);
    std::memcpy(rows, r.data(), r.size() * sizeof(float));
    std::memcpy(cols, c.data(), c.size() * sizeof(float));
    return PRT_OK;
}

extern "C" int prt_set_walk_min_lanes(prt_ctx* c, uint32_t lanes) {
    CTX_CHECK(c);
    if (lanes < 1 || lanes > 64) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_walk_min_lanes: 1..64");
    c->walk_min_lanes = lanes;
    c->shadow_min_lanes = lanes;                    // an explicit setting applies to both kinds of walk phase
    return PRT_OK;
}

// Schedule and build choices of a context.  None of them changes a bit of any result (the tests render the goldens under each);
// they exist for tests, experiments and tuning.  The same names in upper case with the prefix PRT_ are read from the environment
// by prt_create.
extern "C" int prt_set_option(prt_ctx* c, const char* name, int value) {
    CTX_CHECK(c);
    if (!name) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_option: null name");
    const std::string n(name);
    auto bad = [&]() { return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_option: value out of range for " + n); };
    if (n == "waves") { if (value != 0 && value != 5 && value != 6) return bad(); c->lo.waves = value; }
    else if (n == "scatter") { if (value < -1 || value > 1) return bad(); c->lo.scatter = value; }
    else if (n == "generic") { if (value < 0 || value > 1) return bad(); c->lo.generic = value; }
    else if (n == "any_dist") { if (value < 0 || value > 1) return bad(); c->lo.any_dist = value; }
    else if (n == "pix_per_wave") { if (value != 0 && value != 64 && value != 32 && value != 16) return bad(); c->lo.pix_per_wave = value; }
    else if (n == "pool") { if (value < 0 || value > 1) return bad(); c->lo.pool = value; }
    else if (n == "walk_min_lanes") { if (value < 0 || value > 64) return bad(); c->walk_min_lanes = (uint32_t)value; }
    else if (n == "shadow_min_lanes") { if (value < 0 || value > 64) return bad(); c->shadow_min_lanes = (uint32_t)value; }
    else if (n == "tri_q") { if (value < 0 || value > 16) return bad(); c->tri_sixteenths = (uint32_t)value; }
    else if (n == "frames_per_launch") { if (value < 0) return bad(); c->frames_per_launch = (unsigned)value; }
    else if (n == "run_ahead") { if (value < 0 || value > 1) return bad(); c->run_ahead = (uint32_t)value; }
    else if (n == "pace") { if (value < 0 || value > 1) return bad(); c->pace = value; }
    else if (n == "tile_order") {
        if (value < 0 || value > 1) return bad();
        if (value != c->tile_sort) for (int j = 0; j < prt_ctx::MAX_SUB; ++j) c->have_order[j] = false;      // (setting it again keeps a measured order)
        c->tile_sort = value;
    }
    else if (n == "compact") { if (value < 0 || value > 1) return bad(); c->compact = value; }
    else if (n == "compact_below") { if (value < 0 || value > 100) return bad(); c->compact_below = value; }
    else if (n == "test_drop_report") { if (value < 0 || value > 1) return bad(); c->test_drop_report = value != 0; }
    else return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_option: unknown option " + n);
    return PRT_OK;
}

extern "C" const char* prt_kernel_variant(prt_ctx* c) {
    if (!c) return "";
    const RenderLaunch& l = c->last;
    const char* pixels = l.list ? " pixels=live list" : (l.scatter ? " pixels=scattered" : (l.ordered ? " pixels=tiles, expensive first" : " pixels=tiles"));
    std::string name(l.name);
    const size_t f = name.rfind(",filter>");                // the filter builds: the context's kind
    if (f != std::string::npos && c->filter_kind != PRT_FILTER_NONE) name.insert(f + 7, std::string("=") + k_filter_names[c->filter_kind]);
    c->variant = name + (l.waves ? " waves=" + std::to_string(l.waves) + pixels + (l.pix_per_wave != 64 ? ", " + std::to_string(l.pix_per_wave) + " per wave" : "") +
                                        (l.pool ? ", pool" : "") + (l.adaptive ? ", adaptive" : "") : "");
    return c->variant.c_str();
}

extern "C" int prt_synchronize(prt_ctx* c) {
    CTX_CHECK(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->timing_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->stats.kernel_ms = ms;
        if (c->stats.kernel_sum_ms == 0.0) c->stats.kernel_sum_ms = c->stats.kernel_ms;      // launches were not timed one by one
        c->timing_pending = false;
    }
    return PRT_OK;
}

extern "C" int prt_read_framebuffer(prt_ctx* c, float* rgba) {
    CTX_CHECK(c);
    if (!rgba || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_framebuffer: bad arguments");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(rgba, c->fb, c->npix * 16, hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_tonemap_rgba8(prt_ctx* c, uint8_t* rgba) {
    CTX_CHECK(c);
    if (!rgba || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_tonemap_rgba8: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    unsigned char* d = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), c->npix * 4));
    launch_tonemap(c->fb, d, frame_args(c, 1, 0, nullptr, 0, false), c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(rgba, d, c->npix * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHK(c, e);
    return PRT_OK;
}

extern "C" int prt_copy_framebuffer_to_device(prt_ctx* c, void* device_rgba) {
    CTX_CHECK(c);
    if (!device_rgba || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_copy_framebuffer_to_device: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(device_rgba, c->fb, c->npix * 16, hipMemcpyDeviceToDevice, c->stream));
    // on a caller's stream (prt_set_stream) the copy is ordered like any other work of the caller; the context's own
    // stream is private and non-blocking, nothing of the caller's could wait for it: finish the copy before returning
    if (c->stream == c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

extern "C" int prt_read_state(prt_ctx* c, prt_path_state* state) {
    CTX_CHECK(c);
    if (!state || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_state: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    prt_path_state* d = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), c->npix * sizeof(prt_path_state)));
    launch_state_to_rtd(c->S, d, c->npix, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(state, d, c->npix * sizeof(prt_path_state), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHK(c, e);
    return PRT_OK;
}

extern "C" int prt_write_state(prt_ctx* c, const prt_path_state* state) {
    CTX_CHECK(c);
    if (!state || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_write_state: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    prt_path_state* d = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), c->npix * sizeof(prt_path_state)));
    hipError_t e = hipMemcpy(d, state, c->npix * sizeof(prt_path_state), hipMemcpyHostToDevice);
    if (e == hipSuccess) { launch_rtd_to_state(d, c->S, c->fb, c->npix, c->stream); e = hipStreamSynchronize(c->stream); }
    (void)hipFree(d);
    HIPCHK(c, e);
    c->state_undefined = false;
    c->fresh = false;
    c->stats_valid = false;
    return PRT_OK;
}

extern "C" int prt_set_stream(prt_ctx* c, void* hip_stream) {
    CTX_CHECK(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    return PRT_OK;
}

extern "C" int prt_get_stats(prt_ctx* c, prt_stats* out) {
    CTX_CHECK(c);
    if (!out) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_get_stats: null");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    *out = c->stats;
    return PRT_OK;
}

extern "C" int prt_query_counts(prt_ctx* c, uint32_t spp, prt_stats* out) {
    CTX_CHECK(c);
    if (!out || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_query_counts: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->d_counters + 1, 0, 3 * sizeof(unsigned long long), c->stream));
    launch_count(c->S, c->npix, spp, c->d_counters + 1, c->stream);
    unsigned long long h[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->d_counters + 1, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    int rc = prt_synchronize(c);
    if (rc) return rc;
    c->stats.samples = h[0]; c->stats.segments = h[1]; c->stats.finished_pixels = h[2];
    *out = c->stats;
    return PRT_OK;
}

extern "C" int prt_selftest_math(prt_ctx* c, int fn, const float* a, const float* b, float* out, int n) {
    CTX_CHECK(c);
    if (!a || !b || !out || n <= 0) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_selftest_math: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * sizeof(float);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&da), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&db), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dout), bytes);
    if (e == hipSuccess) e = hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) { launch_selftest_math(fn, da, db, dout, n, c->stream); e = hipStreamSynchronize(c->stream); }
    if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
    if (da) (void)hipFree(da);
    if (db) (void)hipFree(db);
    if (dout) (void)hipFree(dout);
    HIPCHK(c, e);
    return PRT_OK;
}

extern "C" int prt_selftest_fn(prt_ctx* c, int fn, const float* params, const float* in, float* out, int n) {
    CTX_CHECK(c);
    if (!params || !in || !out || n <= 0 || fn < 1 || fn > 14) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_selftest_fn: bad arguments");
    const bool env_fn = fn == 13 || fn == 14;                  // environment importance sampling on the uploaded map (pt_selftest.h selftest_env)
    if (env_fn && !(c->sc.env_cdf_rows && c->sc.env_cdf_cols && c->d_env))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_selftest_fn: fn 13 / 14 need a map uploaded to a context created with env_importance_sampling");
    HIPCHK(c, hipSetDevice(c->device));
    float tab[PT_FILTER_TAB + 1] = {};
    float r = 0.0f;
    uint32_t kind = 0;
    if (fn == 12) {                                            // the pixel filter's offsets (pt_filter.hip): params {kind (bits), radius}
        std::memcpy(&kind, params, sizeof(kind));
        if (!filter_radius(kind, params[1], r) || kind == PRT_FILTER_NONE) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_selftest_fn: fn 12 needs a filter kind and radius");
        if (kind >= PRT_FILTER_GAUSSIAN) build_filter_table(kind, r, tab);
    }
    float *dp = nullptr, *di = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * 32 * sizeof(float);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dp), 80 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&di), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dout), bytes);
    if (e == hipSuccess) e = hipMemcpy(dp, params, 80 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(di, in, bytes, hipMemcpyHostToDevice);
    float* dtab = nullptr;
    if (e == hipSuccess && fn == 12) e = hipMalloc(reinterpret_cast<void**>(&dtab), sizeof(tab));
    if (e == hipSuccess && fn == 12) e = hipMemcpy(dtab, tab, sizeof(tab), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (fn == 12) launch_selftest_filter(kind, r, kind >= PRT_FILTER_GAUSSIAN ? dtab : nullptr, di, dout, n, c->stream);
        else if (env_fn) launch_selftest_env(fn, c->sc.env, c->sc.env_w, c->sc.env_h, c->sc.env_cdf_rows, c->sc.env_cdf_cols, di, dout, n, c->stream);
        else launch_selftest_fn(fn, dp, di, dout, n, c->stream);
        e = hipStreamSynchronize(c->stream);
    }
    if (dtab) (void)hipFree(dtab);
    if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
    if (dp) (void)hipFree(dp);
    if (di) (void)hipFree(di);
    if (dout) (void)hipFree(dout);
    HIPCHK(c, e);
    return PRT_OK;
}
