// prt_render.cpp -- headless equivalent of the reference's main() (src/main.cpp:323-485) on top of
// the prt C ABI: same argv flags (-scene -width -height -hdr -alpha), same start-up order
// (scene -> model -> BVH -> buffers -> camera -> kernel args), same per-frame protocol
// (frame counter from 1, two rand() values per frame after two consumed at start-up), with the
// GLFW loop replaced by "-frames N" or "-spp N" (with "-adaptive E [-min-spp M] [-abs-floor F] [-spp-map file.pfm]": adaptive sampling,
// -spp the maximum) and PrtSc replaced by "-out file.{png,hdr,pfm}" (default render.png / render.hdr by -encoder, as saveImage()).
// "-denoise" writes the picture through prt_denoise (guides of "-guide-spp K" samples, default 4; with -adaptive the variance comes from
// the stats plane); "-guides-out base" writes base_albedo.pfm, base_normal.pfm and base_depth.pfm.  "-orbit-frames F -orbit-yaw RAD"
// renders F frames along a yaw orbit (InteractiveCamera::changeYaw by RAD between frames), each -spp fresh paths after a prt_reset, guides and
// prt_denoise_temporal -- the loop of a moving camera -- and writes the last one; "-response FASTCAP,RADIUS,K" runs that loop with
// prt_set_temporal_response on.  "-filter none|box|tent|gaussian|blackman-harris
// [-filter-radius R]" renders through prt_set_pixel_filter (antialiasing; every mode above honours it).
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bvh.h"
#include "camera.h"
#include "host_capi.h"
#include "model_loader.h"
#include "prt.h"
#include "scene.h"

static bool write_pfm(const std::string& path, const std::vector<float>& rgba, int w, int h) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "PF\n%d %d\n-1.0\n", w, h);
    std::vector<float> row((size_t)w * 3);
    for (int y = 0; y < h; ++y) {                    // PFM is bottom-up, and so is the framebuffer (row 0 = lowest scan line)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) row[(size_t)x * 3 + c] = rgba[((size_t)y * w + x) * 4 + c];
        std::fwrite(row.data(), sizeof(float), row.size(), f);
    }
    std::fclose(f);
    return true;
}

// PNG with stored (uncompressed) deflate blocks: no zlib needed.  `rgba` bottom-up, PNG rows are top-down
// (the reference flips on write too, include/GL/cl_gl_interop.h:139).
static bool write_png(const std::string& path, const std::vector<uint8_t>& rgba, int w, int h) {
    static uint32_t crc_table[256];
    static bool have_table = false;
    if (!have_table) {
        for (uint32_t n = 0; n < 256; ++n) { uint32_t c = n; for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; crc_table[n] = c; }
        have_table = true;
    }
    auto crc = [&](const std::vector<uint8_t>& d) { uint32_t c = 0xFFFFFFFFu; for (uint8_t b : d) c = crc_table[(c ^ b) & 0xFF] ^ (c >> 8); return c ^ 0xFFFFFFFFu; };
    auto be32 = [](std::vector<uint8_t>& v, uint32_t x) { v.push_back(x >> 24); v.push_back(x >> 16); v.push_back(x >> 8); v.push_back(x); };
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    auto chunk = [&](const char* type, const std::vector<uint8_t>& data) {
        std::vector<uint8_t> len; be32(len, (uint32_t)data.size());
        std::vector<uint8_t> td(type, type + 4); td.insert(td.end(), data.begin(), data.end());
        std::vector<uint8_t> c; be32(c, crc(td));
        std::fwrite(len.data(), 1, 4, f); std::fwrite(td.data(), 1, td.size(), f); std::fwrite(c.data(), 1, 4, f);
    };
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::fwrite(sig, 1, 8, f);
    std::vector<uint8_t> ihdr; be32(ihdr, (uint32_t)w); be32(ihdr, (uint32_t)h);
    ihdr.insert(ihdr.end(), {8, 6, 0, 0, 0});                     // 8 bit, RGBA
    chunk("IHDR", ihdr);
    std::vector<uint8_t> raw;
    raw.reserve((size_t)h * ((size_t)w * 4 + 1));
    for (int y = h - 1; y >= 0; --y) { raw.push_back(0); raw.insert(raw.end(), rgba.begin() + (size_t)y * w * 4, rgba.begin() + (size_t)(y + 1) * w * 4); }
    std::vector<uint8_t> z = {0x78, 0x01};
    uint32_t a = 1, b = 0;
    for (size_t off = 0; off < raw.size();) {
        const size_t n = std::min<size_t>(65535, raw.size() - off);
        z.push_back(off + n == raw.size() ? 1 : 0);
        z.push_back(n & 0xFF); z.push_back(n >> 8); z.push_back(~n & 0xFF); z.push_back((~n >> 8) & 0xFF);
        z.insert(z.end(), raw.begin() + off, raw.begin() + off + n);
        for (size_t i = off; i < off + n; ++i) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
        off += n;
    }
    be32(z, (b << 16) | a);
    chunk("IDAT", z);
    chunk("IEND", {});
    std::fclose(f);
    return true;
}

#define CHECK(call) do { int rc_ = (call); if (rc_ != PRT_OK) { \
    std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ctx ? prt_last_error(ctx) : prt_last_global_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    int window_width = 1280, window_height = 720;                 // src/main.cpp:55-57
    std::string scene_filepath = "../scenes/cornell.json";        // :90
    std::string models_directory = "../resources/models/";        // :35
    std::string env_map_filepath, out_path;
    int encoder = 0;                                               // { 0: ".png", 1: ".hdr" }, src/main.cpp:365-367
    bool alpha = false;
    uint32_t view = PRT_VIEW_RESULTS;                              // kernels/main.cl:15: a source edit in the reference, a flag here
    unsigned frames = 0, spp = 16;
    float adaptive = -1.0f, abs_floor = 0.0f;                      // -adaptive <rel_err>: prt_render_adaptive between -min-spp and -spp paths
    unsigned min_spp = 16;
    std::string spp_map_path;                                      // -spp-map file.pfm: paths per pixel of the adaptive render
    bool denoise = false;                                          // -denoise: the output goes through prt_denoise
    unsigned guide_spp = 4;                                        // -guide-spp K: guide samples per pixel
    std::string guides_out;                                        // -guides-out base: base_{albedo,normal,depth}.pfm
    unsigned orbit_frames = 0;                                     // -orbit-frames F: F frames through prt_denoise_temporal ...
    float orbit_yaw = 0.0f;                                        // -orbit-yaw RAD: ... RAD of yaw apart
    bool response = false;                                         // -response FASTCAP,RADIUS,K: prt_set_temporal_response for the orbit's frames
    prt_temporal_response resp = {PRT_RESPONSE_DEFAULT_FAST_CAP, PRT_RESPONSE_DEFAULT_RADIUS, PRT_RESPONSE_DEFAULT_K, 0};
    std::string filter = "none";                                   // -filter NAME: the pixel filter (prt_set_pixel_filter)
    float filter_radius = PRT_FILTER_DEFAULT_RADIUS;               // -filter-radius R
    bool pick = false;                                             // -pick X,Y: print the hit of that pixel (prt_cast_pixels) and render nothing
    int pick_x = 0, pick_y = 0;
    int device = 0;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "-scene") scene_filepath = next();
        else if (a == "-width") window_width = std::atoi(next());
        else if (a == "-height") window_height = std::atoi(next());
        else if (a == "-hdr") env_map_filepath = next();
        else if (a == "-alpha") alpha = true;
        else if (a == "-view") { const std::string v = next(); view = v == "normal" ? PRT_VIEW_NORMAL : v == "bvh_hit" ? PRT_VIEW_BVH_HIT : PRT_VIEW_RESULTS; }
        else if (a == "-encoder") encoder = std::atoi(next());
        else if (a == "-models") models_directory = next();
        else if (a == "-frames") frames = (unsigned)std::atoi(next());
        else if (a == "-spp") spp = (unsigned)std::atoi(next());
        else if (a == "-out") out_path = next();
        else if (a == "-adaptive") adaptive = (float)std::atof(next());
        else if (a == "-min-spp") min_spp = (unsigned)std::atoi(next());
        else if (a == "-abs-floor") abs_floor = (float)std::atof(next());
        else if (a == "-spp-map") spp_map_path = next();
        else if (a == "-device") device = std::atoi(next());
        else if (a == "-denoise") denoise = true;
        else if (a == "-guide-spp") guide_spp = (unsigned)std::atoi(next());
        else if (a == "-guides-out") guides_out = next();
        else if (a == "-orbit-frames") orbit_frames = (unsigned)std::atoi(next());
        else if (a == "-orbit-yaw") orbit_yaw = (float)std::atof(next());
        else if (a == "-response") {
            if (std::sscanf(next(), "%u,%u,%f", &resp.fast_cap, &resp.radius, &resp.k) != 3) { std::fprintf(stderr, "-response: needs FASTCAP,RADIUS,K\n"); return 2; }
            response = true;
        }
        else if (a == "-filter") filter = next();
        else if (a == "-filter-radius") filter_radius = (float)std::atof(next());
        else if (a == "-pick") {
            if (std::sscanf(next(), "%d,%d", &pick_x, &pick_y) != 2) { std::fprintf(stderr, "-pick: needs X,Y (full-frame pixel coordinates, framebuffer order)\n"); return 2; }
            pick = true;
        }
    }
    static const char* const filter_names[] = {"none", "box", "tent", "gaussian", "blackman-harris"};
    uint32_t filter_kind = 5;
    for (uint32_t k = 0; k < 5; ++k) if (filter == filter_names[k]) filter_kind = k;
    if (filter_kind == 5) {
        std::fprintf(stderr, "-filter: unknown filter \"%s\" (none, box, tent, gaussian, blackman-harris)\n", filter.c_str());
        return 2;
    }
    prt_ctx* ctx = nullptr;
    try {
        prt::host_scene scene;
        scene.load(scene_filepath);                                // :375-376
        prt_config cfg = scene.make_config(alpha);
        cfg.view_option = view;
        CHECK(prt_create(device, &cfg, &ctx));                     // initOpenCL(), :380

        std::vector<float> vertices4, normals4;
        std::unique_ptr<std::vector<prt::cl_BVHnode>> nodes;
        std::unique_ptr<std::vector<uint64_t>> indices;
        if (scene.BUILD_BVH) {                                     // :401-415
            auto ml = std::make_shared<prt::IO::ModelLoader>();
            if (!ml->ImportFromFile(models_directory + scene.obj_path)) { std::fprintf(stderr, "%s\n", ml->last_error().c_str()); return 1; }
            prt::BVH bvh(ml);
            nodes = bvh.PrepareData();
            indices = bvh.GetPrimitiveIndices();
            ml->flatten(vertices4, normals4);
        }
        prt_scene_desc d;
        std::memset(&d, 0, sizeof(d));
        d.meshes = scene.cpu_meshes.data();                        // :418
        for (int i = 0; i < 8; ++i) d.object_count[i] = scene.object_count[i];
        d.obj_material = &scene.obj_mat;
        if (indices) {
            d.vertices = vertices4.data(); d.normals = normals4.data(); d.primitive_indices = indices->data();
            d.triangle_count = (uint32_t)indices->size(); d.bvh_nodes = nodes->data(); d.bvh_node_count = (uint32_t)nodes->size();
        }
        CHECK(prt_upload_scene(ctx, &d));

        prt::InteractiveCamera ic;                                 // initCamera(), :312-319
        ic.setResolution((float)window_width, (float)window_height);
        ic.setFOVX(45.0f);
        prt::Camera cam;
        ic.buildRenderCamera(&cam);                                // render(), :294-297
        CHECK(prt_set_camera(ctx, &cam));
        if (env_map_filepath == "sky") {                           // no .hdr ships with the reference
            std::vector<float> sky((size_t)1024 * 512 * 3);
            prth_make_sky(1024, 512, sky.data());
            CHECK(prt_upload_envmap(ctx, sky.data(), 1024, 512));
        } else if (!env_map_filepath.empty()) {                    // loadHDR, include/GL/cl_gl_interop.h:77-80
            char herr[256] = "";
            int ew = 0, eh = 0;
            const float* erg = nullptr;
            void* hdr = prth_hdr_load(env_map_filepath.c_str(), &ew, &eh, &erg, herr, sizeof(herr));
            if (!hdr) { std::fprintf(stderr, "-hdr: %s\n", herr); prt_destroy(ctx); return 1; }
            const int rc_env = prt_upload_envmap(ctx, erg, ew, eh);
            prth_hdr_free(hdr);
            CHECK(rc_env);
        }
        CHECK(prt_resize(ctx, window_width, window_height));       // cl_flattenI, :451
        if (filter_kind != PRT_FILTER_NONE) CHECK(prt_set_pixel_filter(ctx, filter_kind, filter_radius));
        if (pick) {                                                // one line on stdout: what is under that pixel (%.9g: the floats round-trip)
            const int32_t xy[2] = {pick_x, pick_y};
            prt_hit h;
            CHECK(prt_cast_pixels(ctx, xy, 1, &h));
            std::printf("pick %d,%d: id=%d tri=%u t=%.9g pos=%.9g,%.9g,%.9g normal=%.9g,%.9g,%.9g u=%.9g v=%.9g backside=%u\n", pick_x, pick_y, (int)h.id,
                        (unsigned)h.tri, (double)h.t, (double)h.pos[0], (double)h.pos[1], (double)h.pos[2], (double)h.normal[0], (double)h.normal[1],
                        (double)h.normal[2], (double)h.u, (double)h.v, (unsigned)(h.flags & 1u));
            prt_destroy(ctx);
            return 0;
        }

        const unsigned max_frames = frames ? frames : spp * (unsigned)(cfg.max_bounces > 8 ? cfg.max_bounces : 8) + 64;
        std::vector<int32_t> seeds((size_t)max_frames * 2);
        prth_seed_pairs(1, max_frames, seeds.data());              // rand() protocol, :226-227,301-302
        std::vector<float> orbit_rgba;
        std::vector<uint8_t> orbit_ldr;
        if (orbit_frames) {                                        // the reference restarts from black on each move (:283-291); here the history carries over
            const size_t npix = (size_t)window_width * window_height;
            orbit_rgba.resize(npix * 4);
            orbit_ldr.resize(npix * 4);
            if (response) CHECK(prt_set_temporal_response(ctx, &resp));
            for (unsigned f = 0; f < orbit_frames; ++f) {
                if (f) {
                    ic.changeYaw(orbit_yaw);
                    ic.buildRenderCamera(&cam);
                    CHECK(prt_set_camera(ctx, &cam));
                }
                CHECK(prt_reset(ctx));
                prth_seed_pairs(1 + f * max_frames, max_frames, seeds.data());
                CHECK(prt_render_spp(ctx, spp, max_frames, seeds.data(), nullptr));
                CHECK(prt_render_guides(ctx, guide_spp));
                const bool last = f + 1 == orbit_frames;
                CHECK(prt_denoise_temporal(ctx, nullptr, nullptr, last ? orbit_rgba.data() : nullptr, last ? orbit_ldr.data() : nullptr));
            }
        } else if (frames) CHECK(prt_render_frames(ctx, 1, frames, seeds.data()));
        else if (adaptive >= 0.0f) {
            const prt_adaptive ad = {std::min(min_spp, spp), spp, adaptive, abs_floor};
            CHECK(prt_render_adaptive(ctx, &ad, max_frames, seeds.data(), nullptr));
        } else CHECK(prt_render_spp(ctx, spp, max_frames, seeds.data(), nullptr));

        std::vector<float> rgba((size_t)window_width * window_height * 4);
        CHECK(prt_read_framebuffer(ctx, rgba.data()));             // saveImage(), include/GL/cl_gl_interop.h:144-160
        prt_stats st;
        CHECK(prt_query_counts(ctx, frames ? 0 : spp, &st));
        std::printf("%dx%d: %llu samples, %llu segments, %.1f ms on the device (%u launches)\n", window_width, window_height,
                    (unsigned long long)st.samples, (unsigned long long)st.segments, st.kernel_ms, st.launches);
        if (!frames && adaptive >= 0.0f) {
            const size_t npix = (size_t)window_width * window_height;
            std::printf("adaptive: %.1f paths per pixel on average (%u ... %u, relative error %g)\n", (double)st.samples / (double)npix,
                        std::min(min_spp, spp), spp, (double)adaptive);
            if (!spp_map_path.empty()) {                           // paths per pixel as a grey PFM (framebuffer order: bottom-up, as PFM)
                std::vector<prt_path_state> state(npix);
                CHECK(prt_read_state(ctx, state.data()));
                std::vector<float> map(npix * 4);
                for (size_t k = 0; k < npix; ++k) map[4 * k] = map[4 * k + 1] = map[4 * k + 2] = (float)state[k].samples;
                if (!write_pfm(spp_map_path, map, window_width, window_height)) { std::fprintf(stderr, "cannot write %s\n", spp_map_path.c_str()); return 1; }
            }
        }
        if (denoise || !guides_out.empty()) CHECK(prt_render_guides(ctx, guide_spp));
        if (!guides_out.empty()) {                                 // the guide plane as three PFMs (framebuffer order: bottom-up, as PFM)
            const size_t npix = (size_t)window_width * window_height;
            std::vector<float> g(npix * 8), alb(npix * 4), nrm(npix * 4), dep(npix * 4);
            CHECK(prt_read_guides(ctx, g.data()));
            for (size_t k = 0; k < npix; ++k)
                for (int c = 0; c < 3; ++c) { alb[4 * k + c] = g[8 * k + c]; nrm[4 * k + c] = g[8 * k + 4 + c]; dep[4 * k + c] = g[8 * k + 7]; }
            const std::pair<const char*, const std::vector<float>*> files[3] = {{"_albedo.pfm", &alb}, {"_normal.pfm", &nrm}, {"_depth.pfm", &dep}};
            for (const auto& f : files)
                if (!write_pfm(guides_out + f.first, *f.second, window_width, window_height)) {
                    std::fprintf(stderr, "cannot write %s\n", (guides_out + f.first).c_str());
                    prt_destroy(ctx);
                    return 1;
                }
        }
        if (denoise && !orbit_frames) CHECK(prt_denoise(ctx, nullptr, rgba.data(), nullptr));       // (the variance source: the stats plane after -adaptive)
        if (orbit_frames) rgba = orbit_rgba;
        // saveImage(), include/GL/cl_gl_interop.h:144-160: -encoder 0 -> render.png (the displayed, tonemapped picture), -encoder 1 ->
        // render.hdr (the linear one); -out <file> picks the name, and the format by its extension (.png / .hdr / .pfm)
        if (out_path.empty()) out_path = encoder == 1 ? "render.hdr" : "render.png";
        auto ends_with = [&](const char* ext) { return out_path.size() > 4 && out_path.compare(out_path.size() - 4, 4, ext) == 0; };
        bool ok;
        if (ends_with(".png")) {                                   // encoder 0 of the reference: the tonemapped picture
            std::vector<uint8_t> ldr((size_t)window_width * window_height * 4);
            if (orbit_frames) ldr = orbit_ldr;
            else if (denoise) CHECK(prt_denoise(ctx, nullptr, nullptr, ldr.data()));
            else CHECK(prt_tonemap_rgba8(ctx, ldr.data()));
            ok = write_png(out_path, ldr, window_width, window_height);
        } else if (ends_with(".hdr")) {                            // encoder 1: the linear picture as Radiance RGBE
            char herr[256] = "";
            ok = prth_hdr_write(out_path.c_str(), rgba.data(), window_width, window_height, 4, 1, herr, sizeof(herr)) == 0;
            if (!ok) std::fprintf(stderr, "%s\n", herr);
        } else {                                                   // the linear picture, lossless
            ok = write_pfm(out_path, rgba, window_width, window_height);
        }
        if (!ok) { std::fprintf(stderr, "cannot write %s\n", out_path.c_str()); return 1; }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        if (ctx) prt_destroy(ctx);
        return 1;
    }
    prt_destroy(ctx);
    return 0;
}
