// prt_api.cpp -- implementation of the C ABI in include/prt.h on top of HIP.
// Replaces the OpenCL host sequence of the reference's src/main.cpp (see prt.h for the
// call-by-call mapping).  No CPU fallback: every entry point needs a HIP device.
// This file: the context, the frame, camera, environment map, pixel filter, options, read-backs and selftests.  The scene calls are in
// prt_api_scene.cpp, what deforms the mesh for them (smooth normals, skin, morph targets) in prt_api_deform.cpp, the render drivers in
// prt_api_render.cpp, the denoiser's in prt_api_denoise.cpp, the ray queries in prt_api_query.cpp; prt_ctx.h is what they share.
#include <cstdlib>

#include "prt_ctx.h"
#include "pt_filter.h"
#include "pt_normals.h"
#include "pt_pack.h"
#include "pt_variant.h"

namespace {
thread_local std::string g_global_error;
}

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
        (e = c->ctx.counters.alloc(4 + 2 * prt_ctx::MAX_SUB)) != hipSuccess ||
        (e = hipMemset(c->ctx.counters, 0, (4 + 2 * prt_ctx::MAX_SUB) * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&c->h_unfinished), (prt_ctx::MAX_SUB + 1) * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming)) != hipSuccess) {
        g_global_error = std::string("prt_create: ") + hipGetErrorString(e);
        prt_destroy(c);
        return PRT_ERR_HIP;
    }
    if (const char* ev = std::getenv("PRT_STREAMS")) { const int k = std::atoi(ev); if (k >= 1 && k <= prt_ctx::MAX_SUB) { c->n_sub = k; c->n_sub_forced = true; } }
    for (int j = 0; j < c->n_sub && c->n_sub > 1; ++j)
        if ((e = hipStreamCreateWithFlags(&c->sub_stream[j], hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreate(&c->sub_ev[j])) != hipSuccess || (e = hipEventCreate(&c->sub_ev0[j])) != hipSuccess) {
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
        if (c->sub_ev[j]) (void)hipEventDestroy(c->sub_ev[j]);
        if (c->sub_ev0[j]) (void)hipEventDestroy(c->sub_ev0[j]);
    }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->h_unfinished) (void)hipHostFree(c->h_unfinished);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                                   // (every device buffer: the context's device is the current one)
}

extern "C" int prt_set_camera(prt_ctx* c, const prt_camera* cam) {
    CTX_CHECK(c);
    if (!cam) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_set_camera: null camera");
    make_dev_camera(*cam, c->cam);
    c->have_cam = true;
    c->frame.guides_valid = false;
    forget_tile_orders(c);      // (tile costs are the view's)
    return PRT_OK;
}

// the map and, for prt_config::env_importance_sampling, its sampling density (pt_kernels.hip build_env_cdf)
static int env_tables(prt_ctx* c, const float* rgb, int w, int h) {
    CtxBuffers& x = c->ctx;
    x.env_rows.reset(); x.env_cols.reset();
    x.env_w = w; x.env_h = h;
    const size_t n = (size_t)w * h * 3;
    HIPCHK(c, x.env.alloc(n));
    HIPCHK(c, hipMemcpy(x.env, rgb, n * sizeof(float), hipMemcpyHostToDevice));
    if (c->cfg.env_importance_sampling) {
        std::vector<float> rows, cols;
        build_env_cdf(rgb, w, h, rows, cols);
        HIPCHK(c, x.env_rows.upload(rows));
        HIPCHK(c, x.env_cols.upload(cols));
    }
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
    c->frame.guides_valid = false;
    c->frame.hist.valid = false;
    const int rc = env_tables(c, rgb, w, h);
    bind(c);
    return rc;
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
    c->frame = Frame{};
    c->npix = 0;
    const size_t npix = (size_t)width * (size_t)rows;
    Frame& f = c->frame;
    DevBuf<float4>* planes[5] = {&f.q0, &f.q1, &f.q2, &f.q3, &f.fb};
    hipError_t e = f.q4.alloc(npix);
    for (int k = 0; k < 5 && e == hipSuccess; ++k) e = planes[k]->alloc(npix);
    const size_t n_tiles_alloc = (size_t)render_tile_count(width, rows);
    for (int j = 0; j < c->n_sub && c->n_sub > 1 && e == hipSuccess; ++j) {
        e = f.tile_order[j].alloc(n_tiles_alloc);
        if (e == hipSuccess) e = f.tile_cost[j].alloc(n_tiles_alloc);
        if (e == hipSuccess) e = hipMemset(f.tile_cost[j], 0, n_tiles_alloc * sizeof(uint32_t));    // (a forced 5-wave build reports no costs: all equal then)
    }
    if (e != hipSuccess) c->frame = Frame{};
    bind(c);
    if (e != hipSuccess) {
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
    HIPCHK(c, hipMemsetAsync(c->frame.fb, 0, c->npix * 16, c->stream));
    if (c->frame.adapt) HIPCHK(c, hipMemsetAsync(c->frame.adapt, 0, c->npix * sizeof(float2), c->stream));
    c->fresh = true;
    c->frame.stats_valid = false;
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
        HIPCHK(c, c->ctx.filter_tab.first_use(PT_FILTER_TAB + 1));
        HIPCHK(c, hipMemcpy(c->ctx.filter_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
    }
    c->filter_kind = kind;
    c->filter_r = r;
    c->frame.guides_valid = false;                               // (the temporal history is kept, as by prt_set_camera)
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

// host only, as prt_env_cdf: no device, no context (the rule: pt_normals.h normals_weld)
extern "C" int prt_weld_corners(const float* vertices, uint32_t T, uint32_t* corner_group, uint32_t* n_groups) {
    if (!vertices || !corner_group || !n_groups || T == 0) { g_global_error = "prt_weld_corners: bad arguments"; return PRT_ERR_INVALID_ARGUMENT; }
    if (!normals_weld(vertices, T, corner_group, n_groups)) {
        g_global_error = "prt_weld_corners: a vertex with a non-finite x, y or z";
        return PRT_ERR_INVALID_ARGUMENT;
    }
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
        if (value != c->tile_sort) forget_tile_orders(c);      // (setting it again keeps a measured order)
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
    HIPCHK(c, hipMemcpy(rgba, c->frame.fb, c->npix * 16, hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_tonemap_rgba8(prt_ctx* c, uint8_t* rgba) {
    CTX_CHECK(c);
    if (!rgba || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_tonemap_rgba8: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<unsigned char> d;
    HIPCHK(c, d.alloc(c->npix * 4));
    launch_tonemap(c->frame.fb, d, frame_args(c, 1, 0, nullptr, 0, false), c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(rgba, d, c->npix * 4, hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_copy_framebuffer_to_device(prt_ctx* c, void* device_rgba) {
    CTX_CHECK(c);
    if (!device_rgba || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_copy_framebuffer_to_device: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(device_rgba, c->frame.fb, c->npix * 16, hipMemcpyDeviceToDevice, c->stream));
    // on a caller's stream (prt_set_stream) the copy is ordered like any other work of the caller; the context's own
    // stream is private and non-blocking, nothing of the caller's could wait for it: finish the copy before returning
    if (c->stream == c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

extern "C" int prt_read_state(prt_ctx* c, prt_path_state* state) {
    CTX_CHECK(c);
    if (!state || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_read_state: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<prt_path_state> d;
    HIPCHK(c, d.alloc(c->npix));
    launch_state_to_rtd(c->S, d, c->npix, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(state, d, c->npix * sizeof(prt_path_state), hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_write_state(prt_ctx* c, const prt_path_state* state) {
    CTX_CHECK(c);
    if (!state || !c->have_size) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_write_state: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<prt_path_state> d;
    HIPCHK(c, d.alloc(c->npix));
    HIPCHK(c, hipMemcpy(d, state, c->npix * sizeof(prt_path_state), hipMemcpyHostToDevice));
    launch_rtd_to_state(d, c->S, c->frame.fb, c->npix, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->state_undefined = false;
    c->fresh = false;
    c->frame.stats_valid = false;
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
    HIPCHK(c, hipMemsetAsync(c->ctx.counters + 1, 0, 3 * sizeof(unsigned long long), c->stream));
    launch_count(c->S, c->npix, spp, c->ctx.counters + 1, c->stream);
    unsigned long long h[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->ctx.counters + 1, sizeof(h), hipMemcpyDeviceToHost, c->stream));
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
    DevBuf<float> da, db, dout;
    const size_t bytes = (size_t)n * sizeof(float);
    HIPCHK(c, da.alloc(n));
    HIPCHK(c, db.alloc(n));
    HIPCHK(c, dout.alloc(n));
    HIPCHK(c, hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(db, b, bytes, hipMemcpyHostToDevice));
    launch_selftest_math(fn, da, db, dout, n, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_selftest_fn(prt_ctx* c, int fn, const float* params, const float* in, float* out, int n) {
    CTX_CHECK(c);
    if (!params || !in || !out || n <= 0 || fn < 1 || fn > 14) return fail(c, PRT_ERR_INVALID_ARGUMENT, "prt_selftest_fn: bad arguments");
    const bool env_fn = fn == 13 || fn == 14;                  // environment importance sampling on the uploaded map (pt_selftest.h selftest_env)
    if (env_fn && !(c->sc.env_cdf_rows && c->sc.env_cdf_cols && c->ctx.env))
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
    DevBuf<float> dp, di, dout, dtab;
    const size_t bytes = (size_t)n * 32 * sizeof(float);
    HIPCHK(c, dp.alloc(80));
    HIPCHK(c, di.alloc((size_t)n * 32));
    HIPCHK(c, dout.alloc((size_t)n * 32));
    HIPCHK(c, hipMemcpy(dp, params, 80 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(di, in, bytes, hipMemcpyHostToDevice));
    if (fn == 12) {
        HIPCHK(c, dtab.alloc(PT_FILTER_TAB + 1));
        HIPCHK(c, hipMemcpy(dtab, tab, sizeof(tab), hipMemcpyHostToDevice));
        launch_selftest_filter(kind, r, kind >= PRT_FILTER_GAUSSIAN ? dtab.get() : nullptr, di, dout, n, c->stream);
    } else if (env_fn) launch_selftest_env(fn, c->sc.env, c->sc.env_w, c->sc.env_h, c->sc.env_cdf_rows, c->sc.env_cdf_cols, di, dout, n, c->stream);
    else launch_selftest_fn(fn, dp, di, dout, n, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return PRT_OK;
}
