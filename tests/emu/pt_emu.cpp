// tests/emu/pt_emu.cpp -- TEST INFRASTRUCTURE, never part of libprt.
//
// The device functions of the product (csrc/hip/pt_device.h: the lane machine, BVH steps, BSDFs, ...) compiled for the
// HOST (-DPT_EMU turns __device__ into __host__ __device__; hipcc --cuda-host-only) and driven by a wave emulator that
// mirrors render_kernel's schedule (pt_render_body.h) over 64 Lane records.  Which <MATS, MEDIUM> instance of the lane machine a render runs
// is the launcher's own choice: select_variant over the variant table of csrc/hip/pt_variant.h, the code launch_render calls.  Two uses, both on
// the CPU (-m "not gpu"):
//   * the refactored per-lane phases == oracle/pt_oracle.c, bit for bit, without a GPU;
//   * schedule independence: with `sched_seed` != 0 the length of every walk phase is drawn at random, which must not
//     change a bit of any pixel (lanes drift in frame number; pixels are independent).
// What this does NOT check is the GPU code generation: that is what the -m gpu parity tests are for.  On the host,
// hw_recip is the IEEE divide it is exhaustively equal to on the device (prt_selftest_math fn 17).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt_device.h"
#include "pt_pack.h"
#include "pt_selftest.h"
#include "pt_variant.h"

using namespace prt;
using namespace prt::dev;

namespace {

struct XorShift {
    uint32_t s;
    uint32_t next() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
};

template <unsigned MATS, bool MEDIUM>
void run_tile(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, int tile_x, int tile_y, prt_path_state* state, float* out_rgba,
              uint32_t sched_seed, std::vector<unsigned>& stack_mem, uint32_t* ahead) {
    Lane L[64];
    bool in_frame[64];
    int gxs[64] = {0}, gys[64] = {0};
    size_t ids[64];
    for (int lane = 0; lane < 64; ++lane) {
        const int lx = tile_x * 8 + (lane & 7), ly = tile_y * 8 + (lane >> 3);
        in_frame[lane] = lx < fa.width && ly < fa.rows;
        if (!in_frame[lane]) continue;
        ids[lane] = (size_t)ly * (size_t)fa.width + (size_t)lx;
        gxs[lane] = lx;
        gys[lane] = fa.row0 + (ly / fa.block_rows * fa.n_parts + fa.part) * fa.block_rows + ly % fa.block_rows;
        Lane& l = L[lane];
        lane_init(l);
        const prt_path_state& r = state[ids[lane]];
        l.origin = F3(r.origin[0], r.origin[1], r.origin[2]); l.t = r.time;
        l.dir = F3(r.dir[0], r.dir[1], r.dir[2]); l.time = r.dist;
        l.mask = F3(r.mask[0], r.mask[1], r.mask[2]); l.total = r.total;
        for (int k = 0; k < 4; ++k) l.acc[k] = r.acc[k];
        l.samples = r.samples;
        l.diff = r.diff; l.spec = r.spec; l.trans = r.trans; l.scatters = r.scatters;
        l.wasSpecular = r.was_specular != 0; l.reset = r.reset != 0;
        if (ahead) l.f = ahead[ids[lane]];
    }
    stack_mem.assign((size_t)sc.stack_levels * 64, 0u);
    XorShift xs{sched_seed ? sched_seed * 2654435761u + (uint32_t)(tile_x * 7919 + tile_y) : 0u};
    if (sched_seed && xs.s == 0) xs.s = 1;
    auto phase_T = [&]() -> unsigned { return sched_seed ? 1u + xs.next() % 64u : fa.walk_min_lanes; };
    TravStack stk[64];
    for (int lane = 0; lane < 64; ++lane) { stk[lane].lds = stack_mem.data() + lane; stk[lane].stride = 64; }

    // one walk phase of the wave (render_kernel B / D)
    auto walk_phase = [&](const bool any_hit, const int walk_stage, const int waiting_stage) {
        Ray wr[64];
        RayPre p[64];
        bool go[64];
        unsigned n_start = 0;
        unsigned n_other = 0;
        for (int lane = 0; lane < 64; ++lane) {
            go[lane] = false;
            if (!in_frame[lane]) continue;
            Lane& l = L[lane];
            const bool walking = l.stage == walk_stage;
            if (walking) {
                wr[lane] = any_hit ? lane_shadow_ray<MEDIUM, (MATS & PT_MATS_ENVIS) != 0>(l) : lane_closest_ray<MEDIUM>(l);
                p[lane] = ray_pre(wr[lane]);
                if (l.fresh) { walk_begin(sc, any_hit, wr[lane], any_hit ? wr[lane].t : PT_INF, p[lane], l.w, stk[lane]); l.fresh = false; }
            }
            go[lane] = walking && !l.w.done;
            n_start += go[lane] ? 1u : 0u;
            n_other += ((walking && l.w.done) || l.stage == waiting_stage) ? 1u : 0u;
        }
        const unsigned T = phase_T();
        const unsigned TQ = sched_seed ? xs.next() % 17u : fa.tri_sixteenths;        // a random share of pending lanes starts the triangle tests
        for (;;) {
            // render_kernel's loop: box steps of the lanes without a pending triangle, then -- once enough of the lanes in the loop
            // have one, or the phase is about to end -- one triangle of every pending lane
            unsigned n_in = 0, n_pend = 0, n_act = 0;
            for (int lane = 0; lane < 64; ++lane) {
                if (!go[lane]) continue;
                ++n_in;
                if (!L[lane].w.pend_count) walk_box(sc, any_hit, wr[lane], p[lane], L[lane].w, stk[lane]);
                if (L[lane].w.pend_count) ++n_pend;
                if (!L[lane].w.done) ++n_act;
            }
            if (!n_in) break;
            const bool cut = n_act < T && n_other + (n_start - n_act) > n_act;      // render_kernel's rule (PT_WAIT_RATIO 1)
            const bool tri = n_pend * 16u >= n_in * TQ || cut;
            for (int lane = 0; lane < 64; ++lane) {
                if (!go[lane]) continue;
                if (tri && L[lane].w.pend_count) walk_tri(sc, any_hit, wr[lane], L[lane].w);
                if (L[lane].w.done) go[lane] = false;
            }
            if (cut) break;
        }
    };

    for (;;) {
        bool any = false, laggards = false;
        bool runnable[64];
        for (int lane = 0; lane < 64; ++lane) laggards |= in_frame[lane] && lane_owes_frames(fa, L[lane]);
        for (int lane = 0; lane < 64; ++lane) {
            runnable[lane] = in_frame[lane] && lane_runnable(fa, L[lane], laggards);
            any |= in_frame[lane] && (runnable[lane] || L[lane].stage != ST_READY);
        }
        if (!any) break;
        for (int lane = 0; lane < 64; ++lane)
            if (runnable[lane]) lane_front<MATS, MEDIUM>(sc, cam, fa, L[lane], gxs[lane], gys[lane]);
        walk_phase(false, ST_WALKC, ST_BACK);
        for (int lane = 0; lane < 64; ++lane)
            if (in_frame[lane] && L[lane].stage == ST_WALKC && L[lane].w.done) lane_closest_done<MATS, MEDIUM>(sc, L[lane]);
        for (int lane = 0; lane < 64; ++lane)
            if (in_frame[lane] && L[lane].stage == ST_BACK) lane_back<MATS, MEDIUM>(sc, L[lane]);
        walk_phase(true, ST_WALKS, ST_FINISH);
        for (int lane = 0; lane < 64; ++lane)
            if (in_frame[lane] && L[lane].stage == ST_WALKS && L[lane].w.done) { L[lane].occluded = L[lane].w.found; L[lane].stage = ST_FINISH; }
        for (int lane = 0; lane < 64; ++lane)
            if (in_frame[lane] && L[lane].stage == ST_FINISH) lane_finish<MATS, MEDIUM>(sc, L[lane]);
    }
    for (int lane = 0; lane < 64; ++lane) {
        if (!in_frame[lane] || !L[lane].f) continue;
        const Lane& l = L[lane];
        prt_path_state& r = state[ids[lane]];
        r.origin[0] = l.origin.x; r.origin[1] = l.origin.y; r.origin[2] = l.origin.z; r.time = l.t;
        r.dir[0] = l.dir.x; r.dir[1] = l.dir.y; r.dir[2] = l.dir.z; r.dist = l.time;
        r.mask[0] = l.mask.x; r.mask[1] = l.mask.y; r.mask[2] = l.mask.z; r.total = l.total;
        for (int k = 0; k < 4; ++k) r.acc[k] = l.acc[k];
        r.samples = l.samples;
        r.diff = (uint16_t)l.diff; r.spec = (uint16_t)l.spec; r.trans = (uint16_t)l.trans; r.scatters = (uint16_t)l.scatters;
        r.was_specular = l.wasSpecular ? 1 : 0; r.reset = l.reset ? 1 : 0;
        if (ahead) {                                             // render_kernel keeps this in DevState::q4.w >> 2
            const bool frozen = fa.spp_limit && l.reset && l.samples >= fa.spp_limit;
            ahead[ids[lane]] = (!frozen && l.f > fa.n_frames) ? l.f - fa.n_frames : 0u;
        }
        const float ns = (MATS & PT_MATS_VIEW) ? 1.0f : (float)l.samples;
        float* px = out_rgba + 4 * ids[lane];
        for (int k = 0; k < 4; ++k) px[k] = l.acc[k] / ns;
    }
}

// the launcher-level choices the emulator has: PT_EMU_GENERIC=1 / PT_EMU_ANY_DIST=1 (prt_set_option "generic" / "any_dist")
const char* g_last_variant = "";           // the row emu_render ran last (emu_last_variant)

LaunchOpts env_launch_opts() {
    const auto on = [](const char* name) { const char* e = std::getenv(name); return (e && e[0] == '1') ? 1 : 0; };
    LaunchOpts lo;
    lo.generic = on("PT_EMU_GENERIC"); lo.any_dist = on("PT_EMU_ANY_DIST");
    return lo;
}

}  // namespace

// same arguments as oracle/pt_oracle.h's pto_job, plus the schedule.  Returns 0, or the prt error code of pack_scene.
// filter_kind / filter_r / filter_tab: prt_set_pixel_filter's state as prt_ctx.h (frame_args) puts it into FrameArgs (tab: T[0 .. 256] of the Gaussian and
// Blackman-Harris kinds, else null).  A kind other than PRT_FILTER_NONE runs the PT_MATS_FILTER rows, and is refused (PRT_ERR_UNSUPPORTED) for
// the configs prt_set_pixel_filter refuses (filter_unsupported).  PT_EMU_GENERIC=1 / PT_EMU_ANY_DIST=1: LaunchOpts::generic / any_dist.
extern "C" int emu_render(const prt_config* cfg, const prt_scene_desc* desc, const prt_camera* camera, const float* env_rgb, int env_w, int env_h,
                          int width, int full_height, int row0, int rows, int block_rows, int n_parts, int part,
                          uint32_t first_frame, uint32_t n_frames, const int32_t* seed_pairs, prt_path_state* state, float* out_rgba,
                          uint32_t spp_limit, uint32_t walk_min_lanes, uint32_t sched_seed, char* err, int err_len,
                          uint32_t seed_frames, uint32_t* ahead,     // ahead != null: FrameArgs::run_ahead, per-pixel frames ahead in / out
                          uint32_t filter_kind, float filter_r, const float* filter_tab) {
    PackedScene ps;
    std::string perr;
    const int rc = pack_scene(*cfg, desc, ps, perr);
    if (rc) {
        if (err && err_len > 0) { std::strncpy(err, perr.c_str(), (size_t)err_len - 1); err[err_len - 1] = 0; }
        return rc;
    }
    DevScene sc = ps.sc;
    sc.pairs = ps.pairs.data(); sc.tri_geom = ps.tg.data(); sc.tri_nrm = ps.tn.data();
    sc.spheres = ps.spheres.data(); sc.quads = ps.quads.data(); sc.sdfs = ps.sdfs.data(); sc.mats = ps.mats.data(); sc.light_tab = ps.light_tab.data();
    static const float black[3] = {0.f, 0.f, 0.f};
    sc.env = env_rgb ? env_rgb : black; sc.env_w = env_rgb ? env_w : 1; sc.env_h = env_rgb ? env_h : 1;
    std::vector<float> cdf_rows, cdf_cols;
    if (cfg->env_importance_sampling) {
        build_env_cdf(sc.env, sc.env_w, sc.env_h, cdf_rows, cdf_cols);
        sc.env_cdf_rows = cdf_rows.data(); sc.env_cdf_cols = cdf_cols.data();
    }
    DevCamera cam{};
    camera_basis(*camera, cam);
    FrameArgs fa{};
    fa.width = width; fa.full_height = full_height; fa.row0 = row0; fa.rows = rows;
    fa.block_rows = block_rows > 0 ? block_rows : 1; fa.n_parts = n_parts > 0 ? n_parts : 1; fa.part = part;
    fa.first_frame = first_frame; fa.n_frames = n_frames; fa.seed_pairs = seed_pairs; fa.spp_limit = spp_limit;
    fa.seed_frames = (ahead && seed_frames > n_frames) ? seed_frames : n_frames; fa.run_ahead = ahead ? 1u : 0u;
    fa.unfinished = nullptr; fa.unfinished_host = nullptr; fa.tile_first = 0; fa.tile_stride = 1;
    fa.walk_min_lanes = walk_min_lanes ? walk_min_lanes : 8;
    fa.tri_sixteenths = 4;
    fa.filter_kind = filter_kind; fa.filter_r = filter_r; fa.filter_tab = filter_tab;
    if (filter_kind != PRT_FILTER_NONE) {
        const char* why = nullptr;
        if (filter_kind > PRT_FILTER_BLACKMAN_HARRIS || !(filter_r >= 0.0f && filter_r <= 4.0f)) why = "pixel filter: unknown kind or radius outside [0, 4]";
        else if ((filter_kind == PRT_FILTER_GAUSSIAN || filter_kind == PRT_FILTER_BLACKMAN_HARRIS) && !filter_tab) why = "pixel filter: the kind needs its table";
        if (why) {
            if (err && err_len > 0) { std::strncpy(err, why, (size_t)err_len - 1); err[err_len - 1] = 0; }
            return PRT_ERR_INVALID_ARGUMENT;
        }
        if (const char* no = filter_unsupported(*cfg)) {
            const std::string msg = std::string("pixel filter: no filter instances are built for ") + no;
            if (err && err_len > 0) { std::strncpy(err, msg.c_str(), (size_t)err_len - 1); err[err_len - 1] = 0; }
            return PRT_ERR_UNSUPPORTED;
        }
    }
    const VariantKey key = {sc.active_mats, sc.dist_mask, sc.n_sdfs, filter_kind, sc.has_medium != 0, sc.view != 0, sc.pick_random_light != 0, sc.env_is != 0};
    const Variant* v = select_variant(key, env_launch_opts());
    g_last_variant = v ? v->name : "";
    decltype(&run_tile<0u, false>) run = nullptr;
#define PT_EMU_VARIANT(file, M, MED, name) if (v && v->mats == (M) && v->medium == (MED)) run = &run_tile<(M), (MED)>;
    PT_VARIANTS(PT_EMU_VARIANT)
#undef PT_EMU_VARIANT
    if (!run) {
        if (err && err_len > 0) { std::strncpy(err, "no row of the variant table for this scene", (size_t)err_len - 1); err[err_len - 1] = 0; }
        return PRT_ERR_UNSUPPORTED;
    }
    std::vector<unsigned> stack_mem;
    const int tiles_x = (width + 7) / 8, tiles_y = (rows + 7) / 8;
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) run(sc, cam, fa, tx, ty, state, out_rgba, sched_seed, stack_mem, ahead);
    return 0;
}

// select_variant (csrc/hip/pt_variant.h) for tests/test_variant_select.py: the index of the row it picks (its MATS, MEDIUM and name out), or -1
extern "C" int emu_select_variant(uint32_t active_mats, int has_medium, uint32_t n_sdfs, int view, int pick_random_light, int env_is, uint32_t dist_mask,
                                  uint32_t filter_kind, int generic, int any_dist, uint32_t* mats, int* medium, const char** name) {
    const VariantKey key = {active_mats, dist_mask, n_sdfs, filter_kind, has_medium != 0, view != 0, pick_random_light != 0, env_is != 0};
    LaunchOpts lo;
    lo.generic = generic; lo.any_dist = any_dist;
    const Variant* v = select_variant(key, lo);
    if (!v) return -1;
    *mats = v->mats; *medium = v->medium ? 1 : 0; *name = v->name;
    return (int)(v - k_variants);
}
extern "C" const char* emu_last_variant() { return g_last_variant; }
// row i of the variant table; returns the number of rows
extern "C" int emu_variant_row(int i, uint32_t* mats, int* medium, const char** name, const char** file) {
    if (i >= 0 && i < k_n_variants) { *mats = k_variants[i].mats; *medium = k_variants[i].medium ? 1 : 0; *name = k_variants[i].name; *file = k_variants[i].file; }
    return k_n_variants;
}

// prt_selftest_fn on the host: the same dispatcher (csrc/hip/pt_selftest.h) compiled for x86-64
extern "C" void emu_selftest_fn(int fn, const float* params, const float* in, float* out, int n) {
    for (int i = 0; i < n; ++i) selftest_fn(fn, params, in + 32 * (size_t)i, out + 32 * (size_t)i);
}
// prt_selftest_fn fn 13 / 14 on the host: selftest_env (csrc/hip/pt_selftest.h) on a map and the tables build_env_cdf makes of it
extern "C" void emu_selftest_env(int fn, const float* rgb, int w, int h, const float* in, float* out, int n) {
    std::vector<float> rows, cols;
    build_env_cdf(rgb, w, h, rows, cols);
    DevScene sc = DevScene();
    sc.env = rgb; sc.env_w = w; sc.env_h = h; sc.env_cdf_rows = rows.data(); sc.env_cdf_cols = cols.data();
    for (int i = 0; i < n; ++i) selftest_env(fn, sc, in + 32 * (size_t)i, out + 32 * (size_t)i);
}
