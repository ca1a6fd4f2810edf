// prt_api_denoise.cpp -- the denoiser's calls of the C ABI (include/prt.h): the a-trous filter and its temporal variant on the context's frame
// and on records, and both histories.
#include <cmath>

#include "prt_ctx.h"

static prt_denoise_params default_denoise_params() {
    return prt_denoise_params{PRT_DENOISE_DEFAULT_PASSES, PRT_DENOISE_VAR_AUTO, PRT_DENOISE_DEFAULT_SIGMA_L, PRT_DENOISE_DEFAULT_SIGMA_N,
                              PRT_DENOISE_DEFAULT_SIGMA_Z, PRT_DENOISE_DEFAULT_SIGMA_A};
}
static prt_temporal_params default_temporal_params() {
    return prt_temporal_params{PRT_TEMPORAL_DEFAULT_ALPHA_COLOR, PRT_TEMPORAL_DEFAULT_ALPHA_MOMENTS, PRT_TEMPORAL_DEFAULT_TAU_Z, PRT_TEMPORAL_DEFAULT_COS_N,
                               PRT_TEMPORAL_DEFAULT_HISTORY_CAP, PRT_TEMPORAL_FEEDBACK_ATROUS};
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

// the context's frame holds a picture and its guides (the filter calls on it, and the export)
static int picture_checks(prt_ctx* c, const std::string& w) {
    if (c->sc.view) return fail(c, PRT_ERR_UNSUPPORTED, w + ": a debug view is not a picture to filter");
    if (!c->frame.guides_valid) return fail(c, PRT_ERR_NOT_READY, w + ": no guides for this scene, camera, map and frame (prt_render_guides)");
    if (c->fresh) return fail(c, PRT_ERR_NOT_READY, w + ": nothing rendered since the reset");
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
    if ((rc = picture_checks(c, w))) return rc;
    const bool stats = c->frame.stats_valid && c->frame.adapt;
    if (p.var_source == PRT_DENOISE_VAR_STATS && !stats)
        return fail(c, PRT_ERR_NOT_READY, w + ": PRT_DENOISE_VAR_STATS needs the last render since the reset to be prt_render_adaptive");
    *spatial = p.var_source == PRT_DENOISE_VAR_SPATIAL || (p.var_source == PRT_DENOISE_VAR_AUTO && !stats);
    return PRT_OK;
}

// the filtered W x H plane `out` to the caller: device_rgba (device memory), rgba (host, prt_read_framebuffer's layout) and rgba8 (host,
// prt_tonemap_rgba8's transform); any may be NULL.  The calls on the context's own frame pass its width and rows: denoise_checks has made
// sure it is the whole frame, whose rows the tonemap maps as those of a W x H frame (one part: global row = local row, whatever block_rows)
static int records_output(prt_ctx* c, const float4* out, int W, int H, void* device_rgba, float* rgba, uint8_t* rgba8) {
    const size_t npix = (size_t)W * (size_t)H;
    if (device_rgba) HIPCHK(c, hipMemcpyAsync(device_rgba, out, npix * 16, hipMemcpyDeviceToDevice, c->stream));
    if (rgba8) {
        FrameArgs fa = frame_args(c, 1, 0, nullptr, 0, false);
        fa.width = W; fa.full_height = H; fa.row0 = 0; fa.rows = H; fa.block_rows = 1; fa.n_parts = 1; fa.part = 0;
        DevBuf<unsigned char> d;
        HIPCHK(c, d.alloc(npix * 4));
        launch_tonemap(out, d, fa, c->stream);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(rgba8, d, npix * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rgba) HIPCHK(c, hipMemcpy(rgba, out, npix * 16, hipMemcpyDeviceToHost));
    return PRT_OK;
}

// a temporal call on an npix-pixel history: what it reads (the half of the last call) and writes (the other half).  The history counts as
// empty until history_commit: a failure in between leaves it empty
static TemporalHistory history_begin(const prt_ctx* c, History& h, size_t npix) {
    float4* half_prev = h.planes + 2 * npix * (size_t)h.cur;           // {c, n} plane, then {m1, m2, v, 0}
    float4* half_next = h.planes + 2 * npix * (size_t)(h.cur ^ 1);
    TemporalHistory t;
    t.cn_prev = half_prev; t.m_prev = half_prev + npix; t.guides_prev = h.guides; t.cam_prev = h.cam; t.valid = h.valid;
    t.cn = half_next; t.m = half_next + npix;
    if (c->response_on) {                                              // (history_buffers has allocated the fast plane)
        t.fast_prev = h.fast + npix * (size_t)h.cur; t.fast = h.fast + npix * (size_t)(h.cur ^ 1);
        t.fast_cap = c->response.fast_cap; t.radius = c->response.radius; t.k = c->response.k;
    }
    h.valid = false;
    return t;
}
// ... and behind its launches: the guides and the camera of this call, and the flip
static int history_commit(prt_ctx* c, History& h, const float4* guides, size_t npix, const DevCamera& cam) {
    HIPCHK(c, hipMemcpyAsync(h.guides, guides, npix * 2 * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    h.cur ^= 1;
    h.cam = cam;
    h.valid = true;
    return PRT_OK;
}
// the four read-backs: the frame history (rec false: of the context's frame part) or the record history (of a W x H frame), and of either
// the history itself -- the last call's half, interleaved per pixel: {c, n}, {m1, m2, v, 0} -- or (response) {f.rgb, flag}: the fast plane's
// colour and the flag from the spare lane of the moments plane, which the history read returns as the 0 it always has
static int read_back(prt_ctx* c, const char* who, bool rec, int W, int H, bool response, float* out) {
    const std::string w(who);
    const History& h = rec ? c->ctx.rec_hist : c->frame.hist;
    if (!out || (rec ? W < 1 || H < 1 : !c->have_size)) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": bad arguments");
    if (response && !c->response_on) return fail(c, PRT_ERR_NOT_READY, w + ": no temporal response is set (prt_set_temporal_response)");
    if (!h.valid || (rec && !h.planes) || (response && !h.fast))
        return fail(c, PRT_ERR_NOT_READY, w + (rec ? ": the record history is empty (prt_denoise_records_temporal)" : ": the history is empty (prt_denoise_temporal)"));
    if (rec && (W != c->ctx.rec_hist_w || H != c->ctx.rec_hist_h)) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": the record history has another size");
    int rc = prt_synchronize(c);
    if (rc) return rc;
    const size_t npix = rec ? (size_t)W * (size_t)H : c->npix;
    const float4* half = h.planes + 2 * npix * (size_t)h.cur;
    std::vector<float4> p(2 * npix);                                    // {c, n} or the fast plane, then the moments
    if (!response) HIPCHK(c, hipMemcpy(p.data(), half, 2 * npix * sizeof(float4), hipMemcpyDeviceToHost));
    else {
        HIPCHK(c, hipMemcpy(p.data(), h.fast + npix * (size_t)h.cur, npix * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(p.data() + npix, half + npix, npix * sizeof(float4), hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < npix; ++k) {
        const float4 a = p[k], b = p[npix + k];
        float* o = out + (response ? 4 : 8) * k;
        o[0] = a.x; o[1] = a.y; o[2] = a.z;
        if (response) o[3] = b.w;
        else { o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = 0.0f; }
    }
    return PRT_OK;
}

// the planes of a filter call on the context's own frame; its buffers on first use: two ping-pong planes and the output plane in dn, the
// Gaussian of v in dn_g
static int frame_planes(prt_ctx* c, FilterPlanes& pl) {
    HIPCHK(c, c->frame.dn.first_use(3 * c->npix));
    HIPCHK(c, c->frame.dn_g.first_use(c->npix));
    float4* dn = c->frame.dn;
    pl = FilterPlanes{c->frame.fb, c->frame.guides, dn, dn + c->npix, c->frame.dn_g, dn + 2 * c->npix, c->width, c->rows};
    return PRT_OK;
}
// ... and on a W x H frame of records, in the context's record block (grown on demand): the framebuffer plane, the guide planes (2), the
// filter's three, the Gaussian of v and, behind it, the "a record without stats" word
static int record_planes(prt_ctx* c, int W, int H, FilterPlanes& pl, unsigned** no_stats) {
    const size_t npix = (size_t)W * (size_t)H;
    HIPCHK(c, c->ctx.rec.reserve(npix * (6 * sizeof(float4) + sizeof(float)) + sizeof(unsigned)));
    float4* fb = reinterpret_cast<float4*>(c->ctx.rec.get());
    float* g = reinterpret_cast<float*>(fb + 6 * npix);
    pl = FilterPlanes{fb, fb + npix, fb + 3 * npix, fb + 4 * npix, g, fb + 5 * npix, W, H};
    *no_stats = reinterpret_cast<unsigned*>(g + npix);
    return PRT_OK;
}
// the two buffers of an npix-pixel history, on first use, and with a temporal response its fast plane (two halves); anew: whatever it holds
// goes first (the record history at a new size)
static int history_buffers(prt_ctx* c, History& h, size_t npix, bool anew) {
    if (anew) h = History{};
    HIPCHK(c, h.planes.first_use(4 * npix));
    HIPCHK(c, h.guides.first_use(2 * npix));
    if (c->response_on) HIPCHK(c, h.fast.first_use(2 * npix));
    return PRT_OK;
}

// the temporal half of a filtering call: its parameters and camera, the history it continues (anew: what that holds goes first) and the
// motion plane of the guides (W x H float4 {D, m}, device) or null
struct TemporalCall { const prt_temporal_params& t; const DevCamera& cam; History& hist; bool anew; const float4* motion; };

// what every filtering door ends in.  pending: the variance step of the frame doors, queued behind the history's allocations (the record
// doors had to run theirs first, for the records' verdict: null)
static int filter_and_output(prt_ctx* c, const FilterPlanes& pl, const VarianceSource* pending, const prt_denoise_params& p, const TemporalCall* tc,
                             void* device_rgba, float* rgba, uint8_t* rgba8) {
    const size_t npix = (size_t)pl.W * (size_t)pl.H;
    TemporalHistory h{};
    if (tc) {
        if (int rc = history_buffers(c, tc->hist, npix, tc->anew)) return rc;
        h = history_begin(c, tc->hist, npix);
    }
    if (pending) launch_filter_variance(pl, tc != nullptr, *pending, c->stream);
    launch_filter_chain(pl, p, tc ? &tc->t : nullptr, tc ? &tc->cam : nullptr, &h, tc ? tc->motion : nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    if (tc)
        if (int rc = history_commit(c, tc->hist, pl.guides, npix, tc->cam)) return rc;
    return records_output(c, pl.out, pl.W, pl.H, device_rgba, rgba, rgba8);
}

extern "C" int prt_denoise(prt_ctx* c, const prt_denoise_params* params, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    const prt_denoise_params p = params ? *params : default_denoise_params();
    VarianceSource src{false, c->S.q4, c->frame.adapt};
    int rc = denoise_checks(c, p, "prt_denoise", &src.spatial);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    FilterPlanes pl;
    if ((rc = frame_planes(c, pl))) return rc;
    return filter_and_output(c, pl, &src, p, nullptr, nullptr, rgba, rgba8);
}

extern "C" int prt_denoise_temporal(prt_ctx* c, const prt_denoise_params* spatial, const prt_temporal_params* temporal, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    const prt_denoise_params p = spatial ? *spatial : default_denoise_params();
    const prt_temporal_params t = temporal ? *temporal : default_temporal_params();
    int rc = temporal_param_checks(c, t, "prt_denoise_temporal");
    if (rc) return rc;
    VarianceSource src{false, c->S.q4, c->frame.adapt};
    rc = denoise_checks(c, p, "prt_denoise_temporal", &src.spatial);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    FilterPlanes pl;
    if ((rc = frame_planes(c, pl))) return rc;
    // the context's motion plane when motion is on and the plane is the valid guides' own (prt.h)
    const TemporalCall tc{t, c->cam, c->frame.hist, false, (c->motion && c->frame.motion_valid) ? c->frame.motion.get() : nullptr};
    return filter_and_output(c, pl, &src, p, &tc, nullptr, rgba, rgba8);
}

extern "C" int prt_read_history(prt_ctx* c, float* out8) {
    CTX_CHECK(c);
    return read_back(c, "prt_read_history", false, 0, 0, false, out8);
}

extern "C" int prt_reset_history(prt_ctx* c) {
    CTX_CHECK(c);
    c->frame.hist.valid = false;
    return PRT_OK;
}

// ---- temporal response (prt.h prt_set_temporal_response; pt_temporal.hip tm_clamp_kernel) ------------------------------------------------------
extern "C" int prt_set_temporal_response(prt_ctx* c, const prt_temporal_response* r) {
    CTX_CHECK(c);
    if (r) {
        if (r->fast_cap < 1 || r->radius < 1 || r->radius > 3 || !(r->k > 0.0f) || !std::isfinite(r->k))
            return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_temporal_response: fast_cap must be >= 1, radius 1 .. 3 and k > 0 and finite");
        if (c->cfg.view_option != PRT_VIEW_RESULTS)
            return fail(c, PRT_ERR_UNSUPPORTED, "prt_set_temporal_response: a debug view is not a picture to filter");
        if (c->response_on && c->response.fast_cap == r->fast_cap && c->response.radius == r->radius && c->response.k == r->k) return PRT_OK;
    } else if (!c->response_on) {
        return PRT_OK;
    }
    // a change: the fast planes hold nothing the new setting could reproject, so both histories start over
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->frame.hist.valid = false;
    c->ctx.rec_hist.valid = false;
    c->response_on = r != nullptr;
    c->response = r ? *r : prt_temporal_response{};
    c->response._pad = 0;
    if (!r) { c->frame.hist.fast.reset(); c->ctx.rec_hist.fast.reset(); }
    return PRT_OK;
}

extern "C" int prt_read_response(prt_ctx* c, float* out4) {
    CTX_CHECK(c);
    return read_back(c, "prt_read_response", false, 0, 0, true, out4);
}

// ---- denoiser inputs as records (prt.h prt_export_denoise_inputs, prt_denoise_records; pt_records.hip) ---------------------------------------
extern "C" int prt_export_denoise_inputs(prt_ctx* c, void* device_records) {
    CTX_CHECK(c);
    if (!device_records || !aligned16(device_records) || !c->have_size)
        return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_export_denoise_inputs: bad arguments (a 16-byte aligned device pointer, a context with a frame size)");
    if (c->state_undefined) return fail(c, PRT_ERR_NOT_READY, "prt_export_denoise_inputs: an earlier render call failed half-way; prt_reset or prt_write_state first");
    if (int rc = picture_checks(c, "prt_export_denoise_inputs")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const bool stats = c->frame.stats_valid && c->frame.adapt;
    launch_records_export(c->frame.fb, c->S.q4, stats ? c->frame.adapt : nullptr, c->frame.guides, c->width, c->rows, static_cast<float4*>(device_records), c->stream);
    HIPCHK(c, hipGetLastError());
    // (prt_copy_framebuffer_to_device: on a caller's stream the records are ordered like the caller's other work; the context's own stream is
    // private: finish before returning)
    if (c->stream == c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// prt_denoise_records (t, cam null) and prt_denoise_records_temporal (device_motion: null, or prt_denoise_records_temporal_motion's plane)
static int denoise_records(prt_ctx* c, const char* who, const prt_denoise_params& p, const prt_temporal_params* t, const prt_camera* cam, int W,
                           int H, const void* device_records, void* device_rgba, float* rgba, uint8_t* rgba8, const void* device_motion = nullptr) {
    const std::string w(who);
    if (W < 1 || H < 1 || !device_records || !aligned16(device_records) || (device_rgba && !aligned16(device_rgba)) || !aligned16(device_motion))
        return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": needs width >= 1, height >= 1 and 16-byte aligned device pointers (records not null)");
    HIPCHK(c, hipSetDevice(c->device));
    FilterPlanes pl;
    unsigned* d_flag = nullptr;
    if (int rc = record_planes(c, W, H, pl, &d_flag)) return rc;
    HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(unsigned), c->stream));
    VarianceSource src;
    src.records = static_cast<const float4*>(device_records); src.no_stats = d_flag;
    launch_filter_variance(pl, t != nullptr, src, c->stream);
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
    if (spatial) launch_filter_variance(pl, t != nullptr, VarianceSource{true}, c->stream);       // the 5x5 moments of the gathered colours
    if (!t) return filter_and_output(c, pl, nullptr, p, nullptr, device_rgba, rgba, rgba8);
    // the record history is this size's from here on: one of another size, or without its buffers, starts anew
    History& rh = c->ctx.rec_hist;
    const bool anew = !rh.planes || !rh.guides || c->ctx.rec_hist_w != W || c->ctx.rec_hist_h != H;
    c->ctx.rec_hist_w = W; c->ctx.rec_hist_h = H;
    DevCamera dc;
    make_dev_camera(*cam, dc);
    const TemporalCall tc{*t, dc, rh, anew, static_cast<const float4*>(device_motion)};
    return filter_and_output(c, pl, nullptr, p, &tc, device_rgba, rgba, rgba8);
}

extern "C" int prt_denoise_records(prt_ctx* c, const prt_denoise_params* params, int width, int height, const void* device_records,
                                   void* device_rgba, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    const prt_denoise_params p = params ? *params : default_denoise_params();
    int rc = denoise_param_checks(c, p, "prt_denoise_records");
    if (rc) return rc;
    return denoise_records(c, "prt_denoise_records", p, nullptr, nullptr, width, height, device_records, device_rgba, rgba, rgba8);
}

extern "C" int prt_denoise_records_temporal_motion(prt_ctx* c, const prt_denoise_params* spatial, const prt_temporal_params* temporal,
                                                   const prt_camera* cam, int width, int height, const void* device_records,
                                                   const void* device_motion, void* device_rgba, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    const prt_denoise_params p = spatial ? *spatial : default_denoise_params();
    const prt_temporal_params t = temporal ? *temporal : default_temporal_params();
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
    c->ctx.rec_hist.valid = false;
    return PRT_OK;
}

extern "C" int prt_read_records_history(prt_ctx* c, int width, int height, float* out8) {
    CTX_CHECK(c);
    return read_back(c, "prt_read_records_history", true, width, height, false, out8);
}

extern "C" int prt_read_records_response(prt_ctx* c, int width, int height, float* out4) {
    CTX_CHECK(c);
    return read_back(c, "prt_read_records_response", true, width, height, true, out4);
}
