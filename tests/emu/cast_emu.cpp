// tests/emu/cast_emu.cpp -- TEST INFRASTRUCTURE, never part of libprt: the per-ray bodies of the ray queries (csrc/hip/pt_cast.h) compiled for
// the host (-DPT_EMU) over a scene packed by pt_pack.cpp, the way pt_emu.cpp sets up DevScene.  64 rays per emulated wave: ray i is lane i % 64
// of wave i / 64, with the wave's own walk stack.  tests/emu/cast_api.py binds it.
//
// sched 0: every lane runs cast_one, the plain per-lane loop.  sched 1: cast_kernel's schedule (pt_cast.hip) -- box steps for the lanes without
// a pending triangle, the triangle unit once a quarter of the lanes still walking have one.  sched >= 2: a random schedule drawn from that seed.
// No bit of a result may depend on it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pt_cast.h"
#include "pt_pack.h"

using namespace prt;
using namespace prt::dev;

namespace {

struct XorShift {
    uint32_t s;
    uint32_t next() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
};

template <bool SDF, bool ANY>
void run_wave(const DevScene& sc, const float4* rays, size_t base, unsigned cnt, const uint32_t* slot_vtx, void* out, uint32_t sched,
              std::vector<unsigned>& stack_mem) {
    stack_mem.assign((size_t)sc.stack_levels * 64, 0u);
    TravStack stk[64];
    for (int lane = 0; lane < 64; ++lane) { stk[lane].lds = stack_mem.data() + lane; stk[lane].stride = 64; }
    if (sched == 0) {
        for (unsigned lane = 0; lane < cnt; ++lane) cast_one<SDF, ANY>(sc, rays, base + lane, slot_vtx, out, stk[lane]);
        return;
    }
    CastLane L[64];
    bool valid[64], in_loop[64];
    for (unsigned lane = 0; lane < cnt; ++lane) {
        valid[lane] = cast_begin(sc, ANY, rays, base + lane, L[lane], stk[lane]);
        in_loop[lane] = !L[lane].w.done;
    }
    XorShift xs{sched * 2654435761u + (uint32_t)base + 1u};
    if (xs.s == 0) xs.s = 1;
    for (;;) {
        unsigned n_in = 0, n_pend = 0, n_stepped = 0;
        for (unsigned lane = 0; lane < cnt; ++lane) {
            if (!in_loop[lane]) continue;
            if (!L[lane].w.pend_count && (sched == 1 || (xs.next() & 3u))) { walk_box(sc, ANY, L[lane].ray, L[lane].p, L[lane].w, stk[lane]); ++n_stepped; }
        }
        for (unsigned lane = 0; lane < cnt; ++lane) {
            if (!in_loop[lane]) continue;
            ++n_in;
            if (L[lane].w.pend_count) ++n_pend;
        }
        if (n_in == 0) break;
        const bool unit = n_pend * 16u >= n_in * 4u;
        for (unsigned lane = 0; lane < cnt; ++lane) {
            if (!in_loop[lane] || !L[lane].w.pend_count) continue;
            // (a random schedule that moved no lane this round tests every pending triangle: the walk ends)
            if (sched == 1 ? unit : ((xs.next() & 1u) || n_stepped == 0)) walk_tri(sc, ANY, L[lane].ray, L[lane].w);
        }
        for (unsigned lane = 0; lane < cnt; ++lane)
            if (in_loop[lane] && L[lane].w.done) in_loop[lane] = false;
    }
    for (unsigned lane = 0; lane < cnt; ++lane) {
        const size_t i = base + lane;
        if (ANY) {
            if (valid[lane]) cast_store_occluded<SDF>(sc, L[lane], static_cast<uint32_t*>(out), i);
            else static_cast<uint32_t*>(out)[i] = 0u;
        } else {
            if (valid[lane]) cast_store_hit<SDF>(sc, L[lane], slot_vtx, static_cast<float4*>(out), i);
            else cast_store_miss(static_cast<float4*>(out), i);
        }
    }
}

void set_err(char* err, int err_len, const std::string& msg) {
    if (err && err_len > 0) { std::strncpy(err, msg.c_str(), (size_t)err_len - 1); err[err_len - 1] = 0; }
}

}  // namespace

// n prt_ray records (16-byte aligned) through the scene of (cfg, desc): any_hit 0: n prt_hit records into out (16-byte aligned), 1: n uint32.
// Returns 0, or the prt error code of pack_scene
extern "C" int cast_emu(const prt_config* cfg, const prt_scene_desc* desc, int any_hit, uint32_t sched, const void* rays, uint32_t n, void* out,
                        char* err, int err_len) {
    PackedScene ps;
    std::string perr;
    const int rc = pack_scene(*cfg, desc, ps, perr);
    if (rc) { set_err(err, err_len, perr); return rc; }
    DevScene sc = ps.sc;
    sc.pairs = ps.pairs.data(); sc.tri_geom = ps.tg.data(); sc.tri_nrm = ps.tn.data();
    sc.spheres = ps.spheres.data(); sc.quads = ps.quads.data(); sc.sdfs = ps.sdfs.data(); sc.mats = ps.mats.data(); sc.light_tab = ps.light_tab.data();
    static const float black[3] = {0.f, 0.f, 0.f};
    sc.env = black; sc.env_w = 1; sc.env_h = 1;
    const uint32_t* slot_vtx = ps.slot_vtx.empty() ? nullptr : ps.slot_vtx.data();
    const float4* r = static_cast<const float4*>(rays);
    std::vector<unsigned> stack_mem;
    for (size_t base = 0; base < n; base += 64) {
        const unsigned cnt = (unsigned)(n - base < 64 ? n - base : 64);
        if (sc.n_sdfs) {
            if (any_hit) run_wave<true, true>(sc, r, base, cnt, slot_vtx, out, sched, stack_mem);
            else run_wave<true, false>(sc, r, base, cnt, slot_vtx, out, sched, stack_mem);
        } else {
            if (any_hit) run_wave<false, true>(sc, r, base, cnt, slot_vtx, out, sched, stack_mem);
            else run_wave<false, false>(sc, r, base, cnt, slot_vtx, out, sched, stack_mem);
        }
    }
    return 0;
}

// the rays of prt_cast_pixels: n (x, y) pairs of a width x full_height frame of `camera` into n prt_ray records (16-byte aligned)
extern "C" void cast_emu_pixel_rays(const prt_camera* camera, int width, int full_height, const int32_t* xy, uint32_t n, void* rays) {
    DevCamera cam{};
    camera_basis(*camera, cam);
    for (uint32_t i = 0; i < n; ++i) cast_pixel_ray(cam, width, full_height, xy, i, static_cast<float4*>(rays));
}

// the root box of the packed scene's tree (min_x max_x min_y max_y min_z max_z), for drawing ray origins
extern "C" int cast_emu_root_box(const prt_config* cfg, const prt_scene_desc* desc, float* box6) {
    PackedScene ps;
    std::string perr;
    const int rc = pack_scene(*cfg, desc, ps, perr);
    if (rc) return rc;
    std::memcpy(box6, ps.root_bounds, 6 * sizeof(float));
    return 0;
}
