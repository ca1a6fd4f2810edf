// prt_api_query.cpp -- the ray queries of the C ABI (include/prt.h): closest hit, occlusion, pixel picking (pt_cast.hip).  Every call reads
// the scene tables and writes nothing of the context but the staging buffers below.
#include "prt_ctx.h"

static_assert(sizeof(prt_ray) == 32 && sizeof(prt_hit) == 48, "prt_ray / prt_hit");

static constexpr uint32_t MAX_RAYS = 1u << 26;

// the refusals every query shares, in the order of prt.h; *nothing: n == 0 (the call succeeds and does nothing)
static int query_checks(prt_ctx* c, const char* who, bool need_frame, const void* in, uint32_t n, const void* out, bool device, bool* nothing) {
    const std::string w(who);
    *nothing = false;
    if (c->state_undefined) return fail(c, PRT_ERR_NOT_READY, w + ": an earlier render call failed half-way; prt_reset or prt_write_state first");
    if (!c->have_scene) return fail(c, PRT_ERR_NOT_READY, w + ": no scene uploaded");
    if (need_frame && !c->have_cam) return fail(c, PRT_ERR_NOT_READY, w + ": no camera set");
    if (need_frame && !c->have_size) return fail(c, PRT_ERR_NOT_READY, w + ": no frame size set");
    if (n == 0) { *nothing = true; return PRT_OK; }
    if (!in || !out) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": null pointer");
    if (n > MAX_RAYS) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": more than 2^26 rays in one call");
    if (device && (!aligned16(in) || !aligned16(out))) return fail(c, PRT_ERR_INVALID_ARGUMENT, w + ": the device buffers must be 16-byte aligned");
    return PRT_OK;
}

// slot_vtx on the device with the first query if no update has put it there (a scene without triangles needs none), then the launch
static int cast_launch(prt_ctx* c, bool any_hit, const void* d_rays, uint32_t n, void* d_out) {
    if (c->scene.n_tris)
        if (int rc = refit_tables(c)) return rc;
    launch_cast(c->sc, any_hit, d_rays, n, c->scene.tree.slot_vtx, d_out, c->stream);
    HIPCHK(c, hipGetLastError());
    return PRT_OK;
}

static int cast_device(prt_ctx* c, const char* who, bool any_hit, const void* d_rays, uint32_t n, void* d_out) {
    bool nothing;
    if (int rc = query_checks(c, who, false, d_rays, n, d_out, true, &nothing)) return rc;
    if (nothing) return PRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = cast_launch(c, any_hit, d_rays, n, d_out)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));       // complete on return: the caller's buffers may be read and reused
    return PRT_OK;
}

static int cast_host(prt_ctx* c, const char* who, bool any_hit, const prt_ray* rays, uint32_t n, void* out) {
    bool nothing;
    if (int rc = query_checks(c, who, false, rays, n, out, false, &nothing)) return rc;
    if (nothing) return PRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t out_bytes = (size_t)n * (any_hit ? sizeof(uint32_t) : sizeof(prt_hit));
    HIPCHK(c, c->ctx.cast_rays.reserve((size_t)n * sizeof(prt_ray)));
    HIPCHK(c, c->ctx.cast_out.reserve(out_bytes));
    HIPCHK(c, hipMemcpyAsync(c->ctx.cast_rays, rays, (size_t)n * sizeof(prt_ray), hipMemcpyHostToDevice, c->stream));
    if (int rc = cast_launch(c, any_hit, c->ctx.cast_rays, n, c->ctx.cast_out)) return rc;
    // (into the caller's memory only once the launch has succeeded)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->ctx.cast_out, out_bytes, hipMemcpyDeviceToHost));
    return PRT_OK;
}

extern "C" int prt_cast_rays(prt_ctx* c, const prt_ray* rays, uint32_t n, prt_hit* hits) {
    CTX_CHECK(c);
    return cast_host(c, "prt_cast_rays", false, rays, n, hits);
}

extern "C" int prt_cast_rays_device(prt_ctx* c, const void* d_rays, uint32_t n, void* d_hits) {
    CTX_CHECK(c);
    return cast_device(c, "prt_cast_rays_device", false, d_rays, n, d_hits);
}

extern "C" int prt_occluded(prt_ctx* c, const prt_ray* rays, uint32_t n, uint32_t* out) {
    CTX_CHECK(c);
    return cast_host(c, "prt_occluded", true, rays, n, out);
}

extern "C" int prt_occluded_device(prt_ctx* c, const void* d_rays, uint32_t n, void* d_out) {
    CTX_CHECK(c);
    return cast_device(c, "prt_occluded_device", true, d_rays, n, d_out);
}

extern "C" int prt_cast_pixels(prt_ctx* c, const int32_t* xy, uint32_t n, prt_hit* hits) {
    CTX_CHECK(c);
    bool nothing;
    if (int rc = query_checks(c, "prt_cast_pixels", true, xy, n, hits, false, &nothing)) return rc;
    if (nothing) return PRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // the staging buffer holds the n rays the generator writes and, behind them, the n (x, y) pairs it reads
    const size_t ray_bytes = (size_t)n * sizeof(prt_ray), xy_bytes = (size_t)n * 2 * sizeof(int32_t), out_bytes = (size_t)n * sizeof(prt_hit);
    HIPCHK(c, c->ctx.cast_rays.reserve(ray_bytes + xy_bytes));
    HIPCHK(c, c->ctx.cast_out.reserve(out_bytes));
    int32_t* d_xy = reinterpret_cast<int32_t*>(c->ctx.cast_rays + ray_bytes);
    HIPCHK(c, hipMemcpyAsync(d_xy, xy, xy_bytes, hipMemcpyHostToDevice, c->stream));
    launch_cast_pixel_rays(c->cam, c->width, c->full_height, d_xy, n, c->ctx.cast_rays, c->stream);
    HIPCHK(c, hipGetLastError());
    if (int rc = cast_launch(c, false, c->ctx.cast_rays, n, c->ctx.cast_out)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(hits, c->ctx.cast_out, out_bytes, hipMemcpyDeviceToHost));
    return PRT_OK;
}
