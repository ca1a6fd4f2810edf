// pt_render.h -- render_kernel (the hot kernel of libprt) and its launcher templates.  Included by the instance files
// pt_inst_*.hip, each of which instantiates launch_variant for its group of rows of the variant table (pt_variant.h: which builds exist
// and which one a launch takes), so that the sets compile in parallel (build.py).  See pt_device.h for the arithmetic contract and the
// lane machine.
//
// Launch geometry: one wave per workgroup, owning an 8x8 pixel tile (primary rays of one wave walk the same BVH nodes), or 64
// pixels of 64 tiles in launches with few rounds of waves; dynamic LDS (DevScene::stack_levels x 256 B per workgroup) holds the
// traversal stacks.  A 1920x1080 frame is 32 400 workgroups >> 256 CUs x 24 resident waves, rendered as two interleaved sets of
// tiles on two streams (prt_api_render.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pt_device.h"
#include "pt_launch.h"
#include "pt_pool.h"
#include "pt_variant.h"

namespace prt {

using namespace dev;

#ifndef PT_WAIT_RATIO
#define PT_WAIT_RATIO 1u    // a walk phase is cut short only while more than this many lanes wait per lane still walking (0: while
                            // any lane waits -- the first form of the rule: 1.3 % slower on cornell, the same on the big mesh)
#endif
// waves per SIMD the register allocator must leave room for: two builds per set, 5 (96 VGPRs) and 6 (80).  The history of these numbers
// is the history of the lane's registers: 4 (128 VGPRs) while the SLP vectorizer paired floats into 64-bit registers; 5
// without it and with the lane's flags as bit-fields of one word; 6 once fields of different phases shared registers, the cached hit
// dropped its position and the walk state its spare words.  Which of the two a launch takes: launch_variant.  7 waves the same as 6
// or worse, 8: -10 ... 20 %.
// LaunchOpts::waves = 5 / 6 forces one build (PT_WAVES / PT_BIG_WAVES; prt_set_option "waves", PRT_WAVES).
#ifndef PT_BIG_WAVES
#define PT_BIG_WAVES 6
#endif
#ifndef PT_WAVES
#define PT_WAVES 5
#endif
#ifndef PT_SUBWAVE_SLOTS
#define PT_SUBWAVE_SLOTS 6144u    // launch_sub_shift: waves the launches in flight may add up to with fewer pixels per wave
#endif
#define PT_BLOCK 64         // threads per workgroup: ONE wave.  A workgroup's slot (LDS, dispatch) frees only when its last wave
                            // ends, and waves over the mesh run ~3x longer than waves over a wall: one-wave groups +4 % over 256

// One wave = one 8x8 tile; every lane runs the lane machine of pt_device.h on its pixel until it has done its n_frames
// segments (or froze).  What is wave-level here is only the SCHEDULE: when the two walk phases of an iteration end.
//   walk phase rule: go on while at least fa.walk_min_lanes (closest-hit phase) / fa.shadow_min_lanes (any-hit phase) lanes
//   are still walking; below that, stop as soon as more lanes wait for the phase to end (they finished their walk in it, or
//   sit in the stage behind it) than walk.  A lane cut off keeps its WalkState and LDS stack and resumes in the same phase
//   of the next iteration.
//   triangle rule: inside a walk phase a lane alternates between box steps (walk_box) and the triangles those found (walk_tri, one
//   per call: pt_device.h "deferred leaves"); the wave runs the triangle unit once fa.tri_sixteenths / 16 of the lanes in the loop
//   have one pending, or when the phase is about to end -- it ran for 1.7 lanes of 64 when every box step carried its own loop.
//   run-ahead ("N spp" launches, fa.run_ahead): a lane that has done its n_frames starts on the next launch's frames for as
//   long as another lane of the wave still owes frames of this one; its lead goes into the state (q4.w >> 2).
// WAVES = waves per SIMD the register allocator leaves room for.
#ifdef PT_PHASE_CLOCKS                    // development builds: cycles of a wave per phase of the iteration (tools/phase_clocks.sh)
__device__ unsigned long long g_phase_clocks[12];    // 0..5, 7 cycles per phase, 6 iterations; 8 most iterations of one wave, 9 longest wave (cycles), 10 waves, 11 idle lane-iterations
#define PT_CLK(k) do { const unsigned long long now_ = __builtin_readcyclecounter(); clk_[k] += now_ - last_; last_ = now_; } while (0)
#else
#define PT_CLK(k) do { } while (0)
#endif

// ORDER: the build that takes its tiles in the launcher's order and reports what they cost (FrameArgs::tile_order / tile_cost).  A build
// of its own because the three lines it adds are not free elsewhere: compiled into every kernel they cost the sets that spill most
// 1.6 ... 3.7 % (rough conductor 10.83 -> 10.46 G segments/s, rough dielectric 7.06 -> 6.95, medium 8.74 -> 8.60; LIGHT|DIFF +-0) -- one more
// scalar register alive through the frame loop -- while the order pays through big trees only (+3 ... 6 %).
template <unsigned MATS, bool MEDIUM, int WAVES, bool ORDER = false>
__global__ __launch_bounds__(PT_BLOCK, WAVES) void render_kernel(const DevScene sc, const DevCamera cam, const DevState S,
                                                                 const FrameArgs fa, float4* __restrict__ fb) {
#define PT_RK_ADAPT 0
#include "pt_render_body.h"
#undef PT_RK_ADAPT
}
// The build of prt_render_adaptive (MATS carries PT_MATS_ADAPT): the same lane machine under the adaptive freeze rule (lane_frozen_adaptive, the
// converged bit as bit 31 of q4.w), the {l, s2} plane updated at every path end -- found at the end of an iteration: the lane's frame count
// moved and its path is reset -- and, with fa.live, the list mapping.  No ORDER build: the tile order is off in adaptive renders.
template <unsigned MATS, bool MEDIUM, int WAVES>
__global__ __launch_bounds__(PT_BLOCK, WAVES) void render_kernel_adaptive(const DevScene sc, const DevCamera cam, const DevState S,
                                                                          const FrameArgs fa, float4* __restrict__ fb) {
    constexpr bool ORDER = false;
#define PT_RK_ADAPT 1
#include "pt_render_body.h"
#undef PT_RK_ADAPT
}

// ---- host-side launchers -------------------------------------------------------------------------------
// tiles (= waves) of this launch, and whether its pixels are scattered over them (render_kernel): on when the launch has few rounds
// of waves -- up to 6 144 tiles, or 24 576 through a tree beyond one XCD's L2, whose expensive tiles are more expensive (1080p: +14 %,
// 3840x2160: -4 %)
static inline unsigned launch_grid(const DevScene& sc, const FrameArgs& fa, const LaunchOpts& lo, bool& scatter) {
    const unsigned tiles_x = ((unsigned)fa.width + 7u) / 8u, tiles_y = ((unsigned)fa.rows + 7u) / 8u;
    const unsigned n_tiles = tiles_x * tiles_y;
    const unsigned grid = fa.tile_first >= n_tiles ? 0u : (n_tiles - fa.tile_first + fa.tile_stride - 1) / fa.tile_stride;   // tiles of this sub-part
    scatter = lo.scatter >= 0 ? lo.scatter != 0 : grid <= (big_tree(sc) ? 24576u : 6144u);
    return grid;
}
// Pixels per wave (FrameArgs::sub_shift).  A launch whose tiles leave wave slots of the chip empty -- one rank's share of a frame
// split N ways, a small frame -- lasts as long as its slowest wave, and a wave as long as its slowest lane's chain of segments (every
// frame of a pixel follows its previous one: DESIGN.md s5); with 32 or 16 pixels per wave the maximum runs over fewer lanes, an
// iteration walks for fewer of them, and the waves that would have idled hold the other halves.  `in_flight`: launches that share the
// chip (the sub-parts of prt_api_render.cpp).  6 144 slots = 256 CUs x 4 SIMDs x 6 waves.
static inline unsigned launch_sub_shift(const LaunchOpts& lo, unsigned grid, unsigned in_flight) {
    if (lo.pix_per_wave == 64) return 0u;
    if (lo.pix_per_wave == 32) return 1u;
    if (lo.pix_per_wave == 16) return 2u;
    // Measured (tools/shard_time.py, one rank's share of the 1080p frame split 8 / 4 / 2 ways, 256 spp): 64 pixels per wave 0.091 / 0.117 /
    // 0.175 s, 32: 0.111 / 0.174 / 0.256 s, 16: 0.158 / 0.267 / 0.418 s -- the chain of a wave's slowest pixel does not get shorter with
    // fewer neighbours (an iteration issues the same instructions whoever takes part), and the extra waves cost issue slots the chip
    // does not have to spare even at an eighth of the frame.  So: never by itself.
    (void)grid; (void)in_flight;
    return 0u;
}
template <unsigned MATS, bool MEDIUM, int WAVES>
static void launch_variant_w(const DevScene& sc, const DevCamera& cam, const DevState& S, const FrameArgs& fa, float4* fb,
                             hipStream_t stream, unsigned grid, bool scatter) {
    const size_t lds = (size_t)sc.stack_levels * PT_BLOCK * sizeof(unsigned);
    static size_t lds_attr = 0;                                  // per template instance
    if (lds > 65536u && lds > lds_attr) {   // only a tree that fills the reference's 64-entry stack to the brim
        if constexpr ((MATS & PT_MATS_ADAPT) != 0u)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&render_kernel_adaptive<MATS, MEDIUM, WAVES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        else
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&render_kernel<MATS, MEDIUM, WAVES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if constexpr (WAVES == PT_BIG_WAVES && !(MATS & PT_MATS_ADAPT)) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&render_kernel<MATS, MEDIUM, WAVES, WAVES == PT_BIG_WAVES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        lds_attr = lds;
    }
    if (!grid) return;
    FrameArgs fb_args = fa;
    fb_args.scatter = scatter ? 1u : 0u;
    grid <<= fb_args.sub_shift;                                  // workgroups = waves: 2^sub_shift per tile
    // walk phases end below this many walking lanes (0 = not set by the caller): 8 (10 / 12: +-0.7 % in either wave-count build; the SDF
    // sets: 10 -3 %); 6 with a medium (8: -1 %) and for scattered pixels, whose waves hold more deep walks (512x512 coat: 6 +4 %).  Shadow rays: in a small tree 99 % end at the root and the
    // rest is shallow -- cutting one off costs its pixel a whole iteration, letting the wave finish them costs a few steps (cornell
    // +3 %); through a big mesh they are as deep as any ray and the bound pays as it does for the closest-hit walks (+14 %).
    // Through a tree beyond one XCD's L2: 20 / 12 (3840x2160 x 512 spp, 4096 frames per launch: 12 / 12 -> 3.84, 16 / 16 -> 3.93, 16 / 12 -> 3.96,
    // 20 / 12 -> 4.02 G segments/s; round 2, 512 frames per launch: 8 -> 2.46, 12 -> 2.52, 16 -> 2.51).
    // A launch that leaves wave slots empty (up to 1.5 rounds of waves in flight: one rank's share of a 1080p frame split 4 or 8 ways) lasts as
    // long as its slowest pixel's chain of segments, and a lane that is cut off needs another iteration of its wave for the same segment: there
    // every walk runs to its end (lock step) -- the share of 8 ranks 0.091 -> 0.077 s, of 4 ranks 0.117 -> 0.108 s, of 2 ranks 0.175 -> 0.209 s, the
    // whole frame 0.286 -> 0.340 s (tools/shard_time.py, 256 spp).  Through a big tree the bound stays (the same sweep: +-2 %, or worse).
    // (with fewer pixels per wave the thresholds shrink with the lanes that can walk at all)
    const bool few_waves = !big_tree(sc) && (unsigned long long)(grid >> fb_args.sub_shift) * (fa.tile_stride ? fa.tile_stride : 1u) <= 9216ull;
    if (!fb_args.walk_min_lanes) fb_args.walk_min_lanes = few_waves ? 1u : max(2u, (big_tree(sc) ? 20u : ((MEDIUM || scatter) ? 6u : 8u)) >> fb_args.sub_shift);
    if (!fb_args.shadow_min_lanes) fb_args.shadow_min_lanes = big_tree(sc) ? max(2u, 12u >> fb_args.sub_shift) : 1u;
    if constexpr ((MATS & PT_MATS_ADAPT) != 0u)                 // (launch_variant: the adaptive build of the set)
        hipLaunchKernelGGL((render_kernel_adaptive<MATS, MEDIUM, WAVES>), dim3(grid), dim3(PT_BLOCK), lds, stream, sc, cam, S, fb_args, fb);
    else if (WAVES == PT_BIG_WAVES && (fb_args.tile_order || fb_args.tile_cost))     // (prt_render_spp asks for it through big trees only)
        hipLaunchKernelGGL((render_kernel<MATS, MEDIUM, WAVES, WAVES == PT_BIG_WAVES>), dim3(grid), dim3(PT_BLOCK), lds, stream, sc, cam, S, fb_args, fb);
    else
        hipLaunchKernelGGL((render_kernel<MATS, MEDIUM, WAVES>), dim3(grid), dim3(PT_BLOCK), lds, stream, sc, cam, S, fb_args, fb);
}
// one row of the variant table (v: the row of <MATS, MEDIUM>): picks the wave-count build and the pixel-to-wave mapping; reports both (RenderLaunch).
// Not inline: the explicit instantiation declarations below keep every translation unit but the row's instance file from compiling its kernels
template <unsigned MATS, bool MEDIUM>
RenderLaunch launch_variant(const Variant& v, const DevScene& sc, const DevCamera& cam, const DevState& S, const FrameArgs& fa, float4* fb,
                            hipStream_t stream, const LaunchOpts& lo) {
    bool scatter;
    const unsigned grid = launch_grid(sc, fa, lo, scatter);
    // Waves per SIMD = which register budget the set runs best at.  6 (80 registers) for the light sets, with a medium, for the raymarched
    // SDF sets and through big trees; 5 (96 registers) for the sets whose 80-register build spills most -- the coat set (68 instead of 152 B
    // of scratch) and the generic dispatch (112 instead of 208 B) -- and for scattered pixels of a small tree (one or two rounds of waves,
    // every wave at its own latency: 512x512 coat +5 %).  Measured at 1080p, 5 against 6 waves: LIGHT|DIFF -6 %, rough conductor -3.6 %,
    // rough dielectric -2.3 %, coat +-0 ... +1.3 %, generic +-0; with a medium -7 %, SDF -15 %.
    // Round 4, the sets outside the BASELINE configs (same call, twice each, 1080p): generic dispatch 5 against 6 waves +8 % (cornell_mixed;
    // 84 instead of 180 B of scratch), generic with a medium +3 % (132 / 200 B), coat +1 %, the raymarched SDF set -8 % (116 / 172 ... 256 B:
    // the raymarcher's latency wants the sixth wave more than its spills cost) -- so the run-time dispatch runs its 96-register build with or
    // without a medium (and with it the debug-view, light-pick and environment-sampling sets, which are that dispatch plus a flag), SDF its 80.
    constexpr bool five = !(MATS & PT_MATS_SDF) && ((MATS & ~PT_MATS_FLAGS) == 0u || (!MEDIUM && (MATS & PRT_MAT_COAT) != 0u));
    const int waves = lo.waves ? lo.waves : (big_tree(sc) ? PT_BIG_WAVES : ((scatter || five) ? PT_WAVES : PT_BIG_WAVES));
    RenderLaunch r;
    r.name = v.name; r.scatter = scatter ? 1 : 0;
    if (fa.adapt) {
        // prt_render_adaptive: ONE build per set (the wave count the set's tile launches take), 64 pixels per wave, no ray pool, no tile order;
        // list launches cover ceil(live_count / 64) waves.  (The debug views are refused by the caller: no adaptive build of them.)
        r.adaptive = 1;
        if constexpr (!(MATS & PT_MATS_VIEW)) {
            constexpr int AW = five ? PT_WAVES : PT_BIG_WAVES;
            FrameArgs fs = fa;
            fs.sub_shift = 0u; fs.tile_order = nullptr; fs.tile_cost = nullptr;
            r.waves = AW; r.list = fa.live ? 1 : 0;
            if (fa.live) { r.scatter = 0; fs.scatter = 0u; }
            const unsigned g = fa.live ? (fa.live_count + 63u) / 64u : grid;
            launch_variant_w<MATS | PT_MATS_ADAPT, MEDIUM, AW>(sc, cam, S, fs, fb, stream, g, fa.live ? false : scatter);
        }
        return r;
    }
    FrameArgs fs = fa;
    fs.sub_shift = lo.pool ? 0u : launch_sub_shift(lo, grid, fa.tile_stride);
    r.pix_per_wave = 64 >> fs.sub_shift;
    r.ordered = (!scatter && fa.tile_order && waves >= PT_BIG_WAVES) ? 1 : 0;
    // render_kernel_rp (pt_pool.h): the same launch -- same tiles or scattered pixels, same order -- with the deep walks on walker waves
    // (not built for the pixel filter: its launches take the kernels below)
    if constexpr (!(MATS & PT_MATS_FILTER)) if (lo.pool) {
        FrameArgs fp = fa;
        fp.scatter = scatter ? 1u : 0u;
        const bool ordered = !scatter && (fa.tile_order || fa.tile_cost);
        const bool ok = ordered ? launch_rp<MATS, MEDIUM, PT_BIG_WAVES, true>(sc, cam, S, fp, fb, stream, grid)
                                : launch_rp<MATS, MEDIUM, PT_BIG_WAVES, false>(sc, cam, S, fp, fb, stream, grid);
        if (ok) { r.waves = PT_BIG_WAVES; r.pool = 1; return r; }
    }
#if defined(PT_DEV_ONE_VARIANT) && !defined(PT_DEV_BOTH_WAVES)
    r.waves = PT_BIG_WAVES;
    launch_variant_w<MATS, MEDIUM, PT_BIG_WAVES>(sc, cam, S, fs, fb, stream, grid, scatter);
#else
    if (waves >= PT_BIG_WAVES) { r.waves = PT_BIG_WAVES; launch_variant_w<MATS, MEDIUM, PT_BIG_WAVES>(sc, cam, S, fs, fb, stream, grid, scatter); }
    else { r.waves = PT_WAVES; launch_variant_w<MATS, MEDIUM, PT_WAVES>(sc, cam, S, fs, fb, stream, grid, scatter); }
#endif
    return r;
}
// every row is instantiated in its instance file and nowhere else: pt_inst_<file>.hip is PT_VARIANTS_<FILE>(PT_INSTANTIATE_VARIANT)
#define PT_VARIANT_ARGS const Variant&, const DevScene&, const DevCamera&, const DevState&, const FrameArgs&, float4*, hipStream_t, const LaunchOpts&
#define PT_EXTERN_VARIANT(file, M, MED, name) extern template RenderLaunch launch_variant<(M), (MED)>(PT_VARIANT_ARGS);
#define PT_INSTANTIATE_VARIANT(file, M, MED, name) template RenderLaunch launch_variant<(M), (MED)>(PT_VARIANT_ARGS);
PT_VARIANTS(PT_EXTERN_VARIANT)

}  // namespace prt
