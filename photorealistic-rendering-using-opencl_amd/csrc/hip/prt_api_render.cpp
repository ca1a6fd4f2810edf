// prt_api_render.cpp -- the render calls of the C ABI (include/prt.h): the three drivers of the megakernel (fixed frames, N spp, adaptive) over
// one launch path, the guide render and the read-backs of guides, motion and the adaptive statistics.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <thread>

#include "prt_ctx.h"
#include "pt_prims.h"

static int ensure_seeds(prt_ctx* c, const int32_t* seed_pairs, size_t n_frames) {
    if (!n_frames) return PRT_OK;
    HIPCHK(c, c->ctx.seeds.reserve(2 * n_frames));
    HIPCHK(c, hipMemcpyAsync(c->ctx.seeds, seed_pairs, n_frames * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // caller may free seed_pairs on return
    return PRT_OK;
}

// 1 / (mean path length of the frame so far) = paths started / segments executed over all pixels (one small reduction over the state planes on
// `stream`, which must be idle -- every caller has just waited for the one launch that was in flight on it); 0 if nothing has been rendered yet
static float inverse_mean_path_length(prt_ctx* c, uint32_t spp, hipStream_t stream) {
    unsigned long long h[3] = {0, 0, 0};
    if (hipMemsetAsync(c->ctx.counters + 1, 0, 3 * sizeof(unsigned long long), stream) != hipSuccess) return 0.0f;
    launch_count(c->S, c->npix, spp, c->ctx.counters + 1, stream);
    if (hipMemcpyAsync(h, c->ctx.counters + 1, sizeof(h), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return 0.0f;
    // (the reference IS the mean: 0.9 / 1.15 / 1.3 / 1.5 / 2 x the mean were all slower)
    return (h[0] && h[1]) ? (float)((double)h[0] / (double)h[1]) : 0.0f;
}

// frames a launch covers: the option, or by tree size (prt_ctx::frames_per_launch has the measurements)
static unsigned frames_per_launch(const prt_ctx* c) { return c->frames_per_launch ? c->frames_per_launch : (big_tree(c->sc) ? 4096u : 512u); }

// sub-parts the megakernel renders this frame part in (1 = one launch covers every tile)
// Sets of tiles rendered side by side on internal streams: 2 (PRT_STREAMS) -- but ONE launch for a SHORT render of a frame whose waves all
// fit on the chip at once (up to 5 120 tiles = one round at 5 waves per SIMD; `frames` = the frames the render is expected to take, at
// most two launches' worth): two half-size launches share the chip unevenly there and the render lasts as long as the slower one (512x512 x
// 64 spp: 19 ... 22 ms beside 21 ... 25 ms; one launch +5 ... 8 %, also at 128 spp; 640x640 and up: two are better or equal).  A LONG render
// of such a frame -- one rank's share of a 1080p frame at 1 024 spp, 16 launches -- wants the two sets: each covers the ends of the
// other's launches (0.375 s against 0.426 s).
static int sub_parts(const prt_ctx* c, unsigned long long frames) {
    if (!(c->n_sub > 1 && c->sub_stream[0])) return 1;
    if (!c->n_sub_forced && render_tile_count(c->width, c->rows) <= 5120u && frames <= 2ull * frames_per_launch(c)) return 1;
    return c->n_sub;
}

// ---- one launch path for the three drivers ---------------------------------------------------------------------------------------------------
// A render call in progress: what prt_render_frames, prt_render_spp and prt_render_adaptive do alike.  Their policy -- which windows of
// frames, who waits for whom -- stays with them.
struct Run {
    prt_ctx* c;
    const char* who;                               // the entry point, for its messages
    uint32_t spp, max_frames;                      // of every window()
    int K = 1;                                     // sub-parts, each on its own stream (1: the caller's stream)
    unsigned step = 0;                             // frames per launch
    bool pacing = false;
    float pace_inv_ref = 0.0f;                     // 1 / (the frame's mean path length): known once the first launch has retired

    hipStream_t stream_of(int j) const { return K > 1 ? c->sub_stream[j] : c->stream; }

    // the prologue up to the seeds; frames_hint: the frames the render is expected to take (sub_parts)
    int begin(const int32_t* seed_pairs, unsigned long long frames_hint) {
        HIPCHK(c, hipSetDevice(c->device));
        c->stats.launches = 0; c->stats.frames = 0; c->stats.kernel_ms = 0.0; c->stats.kernel_sum_ms = 0.0; c->stats.concurrent = 1;
        if (int rc = ensure_seeds(c, seed_pairs, max_frames)) return rc;
        step = frames_per_launch(c);
        K = sub_parts(c, frames_hint);
        // (through a big tree the launches are 4 096 frames and a render is a handful of them: 871 k triangles, 3840x2160 x 2 048 spp 4.35 without, 4.31 with)
        pacing = c->pace && c->run_ahead && !big_tree(c->sc);
        return PRT_OK;
    }
    // ... and from the first timed call on.  zero: the sub-part counters are {unfinished, waves done}; a launch that ended abnormally in an
    // earlier call would have left them non-zero and every later ticket wrong: start from zero, ordered before the fork.  The internal
    // streams start behind everything already queued on the caller's stream
    int fork(bool zero) {
        c->fresh = false;
        c->frame.stats_valid = false;
        c->stats.concurrent = (uint32_t)K;
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        if (zero) HIPCHK(c, hipMemsetAsync(c->ctx.counters + 4, 0, 2 * prt_ctx::MAX_SUB * sizeof(unsigned long long), c->stream));
        if (K > 1) HIPCHK(c, hipEventRecord(c->fork_ev, c->stream));
        for (int j = 0; j < K && K > 1; ++j) HIPCHK(c, hipStreamWaitEvent(c->sub_stream[j], c->fork_ev, 0));
        return PRT_OK;
    }
    // any failure between fork and finish leaves through here: kernels may still be running on the internal streams, the caller's stream
    // must not run ahead of them and the context must stay usable
    int abort(int code, const std::string& msg) {
        for (int j = 0; j < K; ++j) (void)hipStreamSynchronize(stream_of(j));
        (void)hipMemsetAsync(c->ctx.counters + 4, 0, 2 * prt_ctx::MAX_SUB * sizeof(unsigned long long), c->stream);
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        c->state_undefined = true;
        return fail(c, code, msg);
    }
#define SUBCHK(run, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (run).abort(PRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
    // the launch that takes the frames behind f: at most `step` of them (n), with the seeds of all that are left (run-ahead)
    FrameArgs window(uint32_t f, uint32_t& n) const {
        n = (max_frames - f < step) ? max_frames - f : step;
        FrameArgs fa = frame_args(c, 1 + f, n, c->ctx.seeds + 2 * (size_t)f, spp, true);
        fa.seed_frames = max_frames - f; fa.run_ahead = c->run_ahead;
        fa.pace_inv_ref = pacing ? pace_inv_ref : 0.0f;
        return fa;
    }
    // one launch of sub-part j.  The last wave of a launch writes the number of pixels still running to pinned host memory and clears the
    // device counters, so there is no copy or fill kernel between launches (with the other stream's kernel filling the chip those waited
    // ~1.7 ms for a wave slot) and the HIP events around a launch time the kernel alone
    int launch_part(int j, FrameArgs fa) {
        fa.unfinished = c->ctx.counters + 4 + 2 * j;
        fa.unfinished_host = c->h_unfinished + (c->test_drop_report ? prt_ctx::MAX_SUB : j);      // (tests: the report goes astray)
        c->h_unfinished[j] = ~0ull;
        if (K > 1) SUBCHK(*this, hipEventRecord(c->sub_ev0[j], stream_of(j)));
        c->last = c->last_sub[j] = launch_render(c->sc, c->cam, c->S, fa, c->frame.fb, stream_of(j), c->lo);
        if (K > 1) SUBCHK(*this, hipEventRecord(c->sub_ev[j], stream_of(j)));
        ++c->stats.launches;
        return PRT_OK;
    }
    // ... once it is over: its time, and what it reported into `left`.  tag: what the log line calls it
    int retire_part(int j, unsigned long long& left, const char* tag) {
        float ms = 0.f;
        if (K > 1 && hipEventElapsedTime(&ms, c->sub_ev0[j], c->sub_ev[j]) == hipSuccess) c->stats.kernel_sum_ms += ms;
        left = __atomic_load_n(c->h_unfinished + j, __ATOMIC_ACQUIRE);
        if (c->launch_log) std::fprintf(stderr, "prt %s %.3f ms, %llu pixels unfinished\n", tag, ms, left);
        // the host armed the word with ~0 before the launch; the last wave of the launch overwrites it (render_kernel).  A launch whose
        // report never arrived must not be read as 1.8e19 unfinished pixels
        if (left == ~0ull) return abort(PRT_ERR_HIP, std::string(who) + ": a launch ended without reporting its unfinished pixels");
        return PRT_OK;
    }
    // the epilogue: the caller's stream continues behind the internal ones (wait: and the host behind it); f frames were used; unfinished:
    // max_frames ran out first (`msg`)
    int finish(uint32_t f, uint32_t* frames_used, bool unfinished, const char* msg, bool wait = false) {
        for (int j = 0; j < K && K > 1; ++j) {
            HIPCHK(c, hipEventRecord(c->sub_ev[j], c->sub_stream[j]));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->sub_ev[j], 0));
        }
        if (K > 1 && wait) HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        c->timing_pending = true;
        c->stats.frames = f;
        if (frames_used) *frames_used = f;
        if (unfinished) return fail(c, PRT_ERR_NOT_READY, std::string(who) + msg);
        return PRT_OK;
    }
};

extern "C" int prt_render_frames(prt_ctx* c, uint32_t first_frame, uint32_t n_frames, const int32_t* seed_pairs) {
    CTX_CHECK(c);
    int rc = ready(c, "prt_render_frames");
    if (rc) return rc;
    if (first_frame == 0 || (n_frames && !seed_pairs)) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_frames: frames start at 1 and need seed pairs");
    Run run{c, "prt_render_frames", 0, n_frames};
    if ((rc = run.begin(seed_pairs, n_frames)) || !n_frames) return rc;           // (no frames: the stats are zeroed and that is all)
    if ((rc = run.fork(false))) return rc;
    const int K = run.K;
    for (uint32_t f = 0; f < n_frames; f += run.step) {
        const uint32_t n = (n_frames - f < run.step) ? n_frames - f : run.step;
        for (int j = 0; j < K; ++j) {
            FrameArgs fa = frame_args(c, first_frame + f, n, c->ctx.seeds + 2 * (size_t)f, 0, false);
            fa.tile_first = (uint32_t)j; fa.tile_stride = (uint32_t)K;
            c->last = launch_render(c->sc, c->cam, c->S, fa, c->frame.fb, run.stream_of(j), c->lo);
            ++c->stats.launches;
        }
    }
    return run.finish(n_frames, nullptr, false, nullptr);
}

extern "C" int prt_render_spp(prt_ctx* c, uint32_t spp, uint32_t max_frames, const int32_t* seed_pairs, uint32_t* frames_used) {
    CTX_CHECK(c);
    int rc = ready(c, "prt_render_spp");
    if (rc) return rc;
    if (!spp || !max_frames || !seed_pairs) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_render_spp: bad arguments");
    Run run{c, "prt_render_spp", spp, max_frames};
    if ((rc = run.begin(seed_pairs, 8ull * spp))) return rc;            // (a path takes 4.4 ... 7.2 segments on the BASELINE scenes)
    const int K = run.K;
    if ((rc = run.fork(K > 1))) return rc;
    uint32_t f = 0;
    bool exhausted = false;
    if (K == 1) {
        unsigned long long unfinished = 1;
        while (f < max_frames && unfinished) {
            uint32_t n;
            HIPCHK(c, hipMemsetAsync(c->ctx.counters, 0, sizeof(unsigned long long), c->stream));
            const FrameArgs fa = run.window(f, n);
            c->last = launch_render(c->sc, c->cam, c->S, fa, c->frame.fb, c->stream, c->lo);
            ++c->stats.launches;
            f += n;
            HIPCHK(c, hipMemcpyAsync(&unfinished, c->ctx.counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (run.pacing && run.pace_inv_ref == 0.0f && unfinished) run.pace_inv_ref = inverse_mean_path_length(c, spp, c->stream);
        }
        exhausted = unfinished != 0;
    } else {
        // Every sub-part advances on its own stream until its own pixels are frozen, one launch in flight (the other sub-part's kernel
        // covers the host round trip; a second launch queued behind the first measured the same).
        uint32_t fj[prt_ctx::MAX_SUB] = {0, 0, 0, 0};            // frames queued so far
        unsigned retired[prt_ctx::MAX_SUB] = {0, 0, 0, 0};       // launches that are over
        bool in_flight[prt_ctx::MAX_SUB] = {false, false, false, false};
        uint32_t f_done[prt_ctx::MAX_SUB] = {0, 0, 0, 0};        // frames after which the sub-part reported 0
        bool stop[prt_ctx::MAX_SUB] = {false, false, false, false};
        const unsigned n_tiles = render_tile_count(c->width, c->rows);
        const bool sorting = c->tile_sort && big_tree(c->sc);
        for (int j = 0; j < K; ++j) stop[j] = (unsigned)j >= n_tiles;      // a sub-part without tiles has nothing to do
        for (;;) {
            bool progressed = false, busy = false;
            for (int j = 0; j < K; ++j) {
                if (!stop[j] && !in_flight[j] && fj[j] < max_frames) {
                    uint32_t n;
                    FrameArgs fa = run.window(fj[j], n);
                    fa.tile_first = (uint32_t)j; fa.tile_stride = (uint32_t)K;
                    if (sorting && c->frame.tile_cost[j]) {
                        fa.tile_order = c->frame.have_order[j] ? c->frame.tile_order[j] : nullptr;
                        fa.tile_cost = (!c->frame.have_order[j] && retired[j] == 0u) ? c->frame.tile_cost[j] : nullptr;
                    }
                    // (a tile's cost is the maximum over its waves -- atomicMax in the kernel: the measuring launch starts from zero)
                    if (fa.tile_cost) SUBCHK(run, hipMemsetAsync(c->frame.tile_cost[j], 0, (size_t)n_tiles * sizeof(uint32_t), c->sub_stream[j]));
                    if ((rc = run.launch_part(j, fa))) return rc;
                    fj[j] += n;
                    in_flight[j] = true;
                    progressed = true;
                }
                if (in_flight[j]) {
                    busy = true;
                    const hipError_t q = hipEventQuery(c->sub_ev[j]);
                    if (q == hipErrorNotReady) continue;
                    SUBCHK(run, q);
                    char tag[64] = "";
                    if (c->launch_log) std::snprintf(tag, sizeof(tag), "launch: part %d #%u", j, retired[j]);
                    unsigned long long left;
                    if ((rc = run.retire_part(j, left, tag))) return rc;
                    if (sorting && c->frame.tile_cost[j] && !c->frame.have_order[j] && retired[j] == 0u && !c->last_sub[j].scatter && n_tiles > (unsigned)j) {
                        // launch 0 of this sub-part is over and its stream idle: its tiles by run time, longest first, for every launch from here on
                        const unsigned grid = (n_tiles - (unsigned)j + (unsigned)K - 1u) / (unsigned)K;
                        c->h_tile_cost.resize(grid); c->h_tile_order.resize(grid);
                        SUBCHK(run, hipMemcpyAsync(c->h_tile_cost.data(), c->frame.tile_cost[j], grid * sizeof(uint32_t), hipMemcpyDeviceToHost, c->sub_stream[j]));
                        SUBCHK(run, hipStreamSynchronize(c->sub_stream[j]));
                        for (unsigned k = 0; k < grid; ++k) c->h_tile_order[k] = k;
                        const uint32_t* cost = c->h_tile_cost.data();
                        std::stable_sort(c->h_tile_order.begin(), c->h_tile_order.end(), [cost](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
                        SUBCHK(run, hipMemcpyAsync(c->frame.tile_order[j], c->h_tile_order.data(), grid * sizeof(uint32_t), hipMemcpyHostToDevice, c->sub_stream[j]));
                        SUBCHK(run, hipStreamSynchronize(c->sub_stream[j]));      // (the host vector is reused by the other sub-part)
                        c->frame.have_order[j] = true;
                    }
                    // the frame's mean path length, once per render (this sub-part's stream is idle: its launch has just retired)
                    if (run.pacing && run.pace_inv_ref == 0.0f && left) run.pace_inv_ref = inverse_mean_path_length(c, spp, c->sub_stream[j]);
                    ++retired[j];
                    in_flight[j] = false;
                    progressed = true;
                    if (left == 0) { stop[j] = true; f_done[j] = fj[j]; }
                    else if (fj[j] >= max_frames) { stop[j] = true; f_done[j] = max_frames; exhausted = true; }
                }
            }
            if (!busy && !progressed) break;
            if (!progressed) std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        for (int j = 0; j < K; ++j) f = f_done[j] > f ? f_done[j] : f;
    }
    return run.finish(f, frames_used, exhausted, ": max_frames reached before every pixel finished", true);
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
    c->arep = prt_adaptive_report{};
    Run run{c, "prt_render_adaptive", a->max_spp, max_frames};
    if ((rc = run.begin(seed_pairs, 8ull * a->max_spp))) return rc;
    const unsigned n_waves = (unsigned)((c->npix + 63) / 64);
    if (!c->frame.adapt) {
        HIPCHK(c, c->frame.adapt.alloc(c->npix));
        HIPCHK(c, hipMemsetAsync(c->frame.adapt, 0, c->npix * sizeof(float2), c->stream));
    }
    HIPCHK(c, c->frame.live.first_use(c->npix));
    HIPCHK(c, c->frame.live_aux.first_use(n_waves + 1));
    if ((rc = run.fork(true))) return rc;
    c->frame.stats_valid = true;                       // (prt_denoise PRT_DENOISE_VAR_STATS)
    const int K = run.K;
    const unsigned n_tiles = render_tile_count(c->width, c->rows);
    bool done[prt_ctx::MAX_SUB] = {false, false, false, false};     // tile rounds: every pixel of the sub-part's tiles is frozen
    for (int j = 0; j < K; ++j) done[j] = (unsigned)j >= n_tiles;
    unsigned long long live = c->npix;
    uint32_t list_count = 0;
    bool list_mode = false;
    uint32_t f = 0;
    while (f < max_frames && live) {
        if (c->compact && live * 100ull < (unsigned long long)c->npix * (unsigned)c->compact_below && (!list_mode || 2ull * live < list_count)) {
            // (every stream is idle: the last round has been waited for)
            launch_live_list(c->S, c->npix, a->max_spp, c->frame.live_aux, c->frame.live, c->frame.live_aux + n_waves, c->stream);
            uint32_t cnt = 0;
            SUBCHK(run, hipMemcpyAsync(&cnt, c->frame.live_aux + n_waves, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
            SUBCHK(run, hipStreamSynchronize(c->stream));
            if (cnt != live) return run.abort(PRT_ERR_HIP, "prt_render_adaptive: the live-pixel list disagrees with the launches' reports");
            list_count = cnt; list_mode = true;
            ++c->arep.list_builds;
        }
        const uint32_t chunk = list_mode ? (((list_count + 63u) / 64u + (uint32_t)K - 1u) / (uint32_t)K) * 64u : 0u;   // (whole waves per sub-part)
        bool launched[prt_ctx::MAX_SUB] = {false, false, false, false};
        uint32_t n = 0;
        for (int j = 0; j < K; ++j) {
            FrameArgs fa = run.window(f, n);
            fa.adapt = c->frame.adapt; fa.min_spp = a->min_spp; fa.rel_err = a->rel_err; fa.abs_floor = a->abs_floor;
            if (list_mode) {
                const uint32_t start = (uint32_t)j * chunk;
                if (start >= list_count) continue;
                fa.live = c->frame.live + start;
                fa.live_count = std::min(chunk, list_count - start);
                c->arep.list_lanes += 64ull * ((fa.live_count + 63u) / 64u);
                ++c->arep.list_launches;
            } else {
                if (done[j]) continue;
                fa.tile_first = (uint32_t)j; fa.tile_stride = (uint32_t)K;
                ++c->arep.tile_launches;
            }
            if ((rc = run.launch_part(j, fa))) return rc;
            launched[j] = true;
        }
        if (list_mode) c->arep.list_live_lanes += live;
        SUBCHK(run, hipGetLastError());
        live = 0;
        for (int j = 0; j < K; ++j) {
            if (!launched[j]) continue;
            SUBCHK(run, hipStreamSynchronize(run.stream_of(j)));
            char tag[96] = "";
            if (c->launch_log) std::snprintf(tag, sizeof(tag), "adaptive launch: part %d frames %u..%u %s", j, 1 + f, f + n, list_mode ? "list" : "tiles");
            unsigned long long left;
            if ((rc = run.retire_part(j, left, tag))) return rc;
            if (!list_mode) done[j] = left == 0;
            live += left;
        }
        f += n;
        if (run.pacing && run.pace_inv_ref == 0.0f && live) run.pace_inv_ref = inverse_mean_path_length(c, a->max_spp, c->stream);
    }
#undef SUBCHK
    return run.finish(f, frames_used, live != 0, ": max_frames reached before every pixel froze");
}

extern "C" int prt_read_adaptive_stats(prt_ctx* c, float* out2) {
    CTX_CHECK(c);
    if (!out2 || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_adaptive_stats: bad arguments");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    if (!c->frame.adapt) { std::memset(out2, 0, c->npix * 2 * sizeof(float)); return PRT_OK; }    // (no adaptive render since the frame was made)
    HIPCHK(c, hipMemcpy(out2, c->frame.adapt, c->npix * sizeof(float2), hipMemcpyDeviceToHost));
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
    c->frame.guides_valid = false;
    c->frame.motion_valid = false;
    HIPCHK(c, c->frame.guides.first_use(2 * c->npix));
    if (c->motion) HIPCHK(c, c->frame.motion.first_use(c->npix));
    const bool snap = c->motion && c->scene.snap.snap_valid && c->scene.snap.tri_prev;
    // the motion instances only where there is a snapshot to measure from; no update since the last guide render: the plain kernels and a
    // plane of zeros
    // ... and the primitive-motion instances only while a primitive snapshot is pending (prt_update_primitives), with the triangle term only
    // while a triangle snapshot is pending too: the two snapshots are independent of each other
    const bool prim_snap = c->motion && c->scene.snap.prim_snap_valid && c->scene.snap.spheres_prev && c->scene.snap.sdfs_prev && c->scene.snap.quads_prev;
    const PrimPrev prims{c->scene.snap.spheres_prev, c->scene.snap.sdfs_prev, c->scene.snap.quads_prev};
    launch_guides(c->sc, c->cam, frame_args(c, 1, 0, nullptr, 0, false), samples, c->frame.guides, snap ? c->scene.snap.tri_prev.get() : nullptr,
                  prim_snap ? &prims : nullptr, c->frame.motion, c->stream);
    HIPCHK(c, hipGetLastError());
    if (c->motion && !snap && !prim_snap) HIPCHK(c, hipMemsetAsync(c->frame.motion, 0, c->npix * sizeof(float4), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->frame.guides_valid = true;
    if (c->motion) {
        c->scene.snap.snap_valid = false;                         // consumed: the next plane is measured from the geometry these guides saw
        c->scene.snap.prim_snap_valid = false;
        c->frame.motion_valid = true;
    }
    return PRT_OK;
}

static int motion_ready(prt_ctx* c, const char* who) {
    const std::string w(who);
    if (!c->motion) return fail(c, PRT_ERR_NOT_READY, w + ": motion is off (prt_set_motion)");
    if (!c->frame.guides_valid || !c->frame.motion_valid || !c->frame.motion)
        return fail(c, PRT_ERR_NOT_READY, w + ": no guides with a motion plane for this scene, camera, map and frame (prt_render_guides)");
    return PRT_OK;
}

extern "C" int prt_read_motion(prt_ctx* c, float* out4) {
    CTX_CHECK(c);
    if (!out4 || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_motion: bad arguments");
    int rc = motion_ready(c, "prt_read_motion");
    if (rc) return rc;
    if ((rc = prt_synchronize(c))) return rc;
    HIPCHK(c, hipMemcpy(out4, c->frame.motion, c->npix * sizeof(float4), hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_export_motion(prt_ctx* c, void* device_motion) {
    CTX_CHECK(c);
    if (!device_motion || !aligned16(device_motion) || !c->have_size)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_export_motion: bad arguments (a 16-byte aligned device pointer, a context with a frame size)");
    int rc = motion_ready(c, "prt_export_motion");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(device_motion, c->frame.motion, c->npix * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    if (c->stream == c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));       // (as prt_export_denoise_inputs)
    return PRT_OK;
}

extern "C" int prt_read_guides(prt_ctx* c, float* out8) {
    CTX_CHECK(c);
    if (!out8 || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_guides: bad arguments");
    if (!c->frame.guides_valid) return fail(c, PRT_ERR_NOT_READY, "prt_read_guides: no guides for this scene, camera, map and frame (prt_render_guides)");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out8, c->frame.guides, c->npix * 2 * sizeof(float4), hipMemcpyDeviceToHost));
    return PRT_OK;
}
