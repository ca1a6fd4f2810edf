// pt_render_body.h -- the body of render_kernel, included twice by pt_render.h: PT_RK_ADAPT 0 for render_kernel, 1 for
// render_kernel_adaptive (prt_render_adaptive).  One text for both, and the "N spp" / frame-mode kernel compiles from exactly the tokens it
// had before the adaptive one existed: rewriting its body with `if constexpr` branches of the adaptive build moved the register allocator's
// spills in 14 of its instances (the view set 236 -> 196 B of scratch, generic 220 -> 204, SDF 84 -> 108) without changing a line it ran.
// No include guard: included inside a function body.
    const int tiles_x = (fa.width + 7) / 8;
    const int lane = threadIdx.x & 63;
    // fa.scatter: the wave's 64 pixels come from 64 tiles spread over the launch's share of the frame instead of one 8x8 tile.
    // Every wave then gets its share of the expensive regions: a launch with few rounds of waves no longer waits for the
    // tiles over the mesh (512x512: +39 %); a big frame loses the coherence of neighbouring pixels' first segments (-17 %).
    // (not scattered: one tile per wave, and which one is the launcher's choice -- FrameArgs::tile_order)
    // fa.sub_shift: the wave renders P = 64 >> sub_shift pixels, 2^sub_shift waves share a tile (or, scattered, the launch's pixels)
    const unsigned P = 64u >> fa.sub_shift;
    const unsigned tile_g = blockIdx.x >> fa.sub_shift;
    const unsigned tile_k = (ORDER && !fa.scatter && fa.tile_order) ? fa.tile_order[tile_g] : tile_g;
    // What a tile costs is reported as the wave's ITERATIONS, not its clock ticks: a time stamp taken here (`s_memtime`, as intrinsic or as
    // inline assembly) counts for the compiler as something every later load may depend on, and such a load cannot go through the scalar
    // cache -- the quads, spheres, materials and the root of the tree all came through the vector-memory path in the first build of this
    // (2.2 x its instructions, 6 % of the scalar loads left; found with the instruction counters, the clock said +-0).
    unsigned iterations = 0u;
    const unsigned vpix = fa.scatter ? (unsigned)lane * gridDim.x + blockIdx.x : tile_k * 64u + (blockIdx.x & ((1u << fa.sub_shift) - 1u)) * P + (unsigned)lane;
    const unsigned tile = (vpix >> 6) * fa.tile_stride + fa.tile_first;
    const int tl = (int)(vpix & 63u);
    const int tile_x = (int)(tile % (unsigned)tiles_x), tile_y = (int)(tile / (unsigned)tiles_x);
#if !PT_RK_ADAPT
    const int lx = tile_x * 8 + (tl & 7);
    const int ly = tile_y * 8 + (tl >> 3);
    // a lane outside the frame (edge tiles) idles through the kernel: every wave reaches the end, where the last one reports
    const bool in_frame = (unsigned)lane < P && lx < fa.width && ly < fa.rows;
#else
    // list launches (fa.live: prt_render_adaptive once few pixels are left): the live pixels in increasing order, 64 to a wave (sub_shift 0)
    const unsigned li = blockIdx.x * 64u + (unsigned)lane;
    const unsigned lp = (fa.live && li < fa.live_count) ? fa.live[li] : 0u;
    const int lx = fa.live ? (int)(lp % (unsigned)fa.width) : tile_x * 8 + (tl & 7);
    const int ly = fa.live ? (int)(lp / (unsigned)fa.width) : tile_y * 8 + (tl >> 3);
    const bool in_frame = fa.live ? li < fa.live_count : ((unsigned)lane < P && lx < fa.width && ly < fa.rows);
#endif
    const size_t id = in_frame ? (size_t)ly * (size_t)fa.width + (size_t)lx : 0;
    const int gx = lx;
    const int gy = fa.row0 + (ly / fa.block_rows * fa.n_parts + fa.part) * fa.block_rows + ly % fa.block_rows;

    Lane L;
    lane_init(L);
#if PT_RK_ADAPT
    L.conv = false;
#endif
    unsigned target = fa.n_frames;                              // frames this lane owes the launch
    if (!in_frame) { L.f = 0xffffffffu; L.reset = true; L.samples = 0xffffffffu; L.wasSpecular = false; }   // owes no frame, starts none
    else {
        const float4 a = S.q0[id], b = S.q1[id], c = S.q2[id], d = S.q3[id];
        const uint4 e = S.q4[id];
        L.origin = F3(a.x, a.y, a.z); L.t = a.w;                // TempRay.time = ray.t of the last segment (main.cl:28)
        L.dir = F3(b.x, b.y, b.z); L.time = b.w;                // TempRay.dist = ray.time
        L.mask = F3(c.x, c.y, c.z); L.total = prt_f2u(c.w);
        L.acc[0] = d.x; L.acc[1] = d.y; L.acc[2] = d.z; L.acc[3] = d.w;
        L.samples = e.x;
        L.diff = e.y & 0xffffu; L.spec = e.y >> 16;
        L.trans = e.z & 0xffffu; L.scatters = e.z >> 16;
        L.wasSpecular = (e.w & 1u) != 0; L.reset = (e.w & 2u) != 0;
#if !PT_RK_ADAPT
        L.f = fa.run_ahead ? e.w >> 2 : 0u;                     // frames of this launch done in an earlier one ("N spp" launches only)
#else
        L.f = fa.run_ahead ? (e.w >> 2) & 0x1fffffffu : 0u;     // (bit 31: the converged bit)
        L.conv = (e.w >> 31) != 0u;
#endif
        // the pace of this pixel: its own mean path length so far (segments / paths started) over the frame's (FrameArgs::pace_inv_ref)
        if (fa.pace_inv_ref > 0.0f && e.x >= 8u) {
            // (cumulative: after this launch the pixel should have done pace x the frames of the launches so far; its lead L.f counts towards that)
            const float pace = fminf(fmaxf(d.w / (float)e.x * fa.pace_inv_ref, 1.0f), 3.0f);
            target = min(fa.n_frames + (unsigned)((pace - 1.0f) * (float)(fa.first_frame - 1u + fa.n_frames)), fa.seed_frames);
        }
    }
    extern __shared__ unsigned lds_stack[];                     // sc.stack_levels x PT_BLOCK, sized by the launch
    TravStack stk;
    stk.lds = lds_stack + threadIdx.x; stk.stride = PT_BLOCK;
    const unsigned T = fa.walk_min_lanes, TD = fa.shadow_min_lanes, TQ = fa.tri_sixteenths;
#ifdef PT_TEST_CLOBBER
    // tests/test_codegen.py: what a time stamp, an `asm volatile` or an LDS atomic in front of the frame loop is to the compiler -- a
    // write that every later load may depend on.  The uniform loads of the kernel must stay scalar behind it (pt_device.h, PT_CONST).
    asm volatile("" ::: "memory");
    atomicAdd(&lds_stack[0], 1u);
#endif
#ifdef PT_PHASE_CLOCKS
    unsigned long long clk_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last_ = __builtin_readcyclecounter();
    const unsigned long long start_ = last_;
    unsigned long long done_lanes_ = 0;
#endif
    for (;;) {
#if !PT_RK_ADAPT
        const bool runnable = lane_runnable(fa, L, __any(lane_owes_frames(fa, L, target)), target);
#else
        const bool runnable = lane_runnable_adaptive(fa, L, __any(lane_owes_frames_adaptive(fa, L, target)), target);
#endif
        if (!__any(runnable || L.stage != ST_READY)) break;     // every lane has done its frames (or is frozen)
#if PT_RK_ADAPT
        const unsigned f_iter = L.f;                            // (a lane ends at most one segment per iteration: in A, or in E)
#endif
        if (ORDER) ++iterations;
        PT_CLK(7);
#ifdef PT_PHASE_CLOCKS
        done_lanes_ += (unsigned long long)__popcll(__ballot(!runnable && L.stage == ST_READY));
#endif
        if (runnable) { PT_WSTAT(4); lane_front<MATS, MEDIUM>(sc, cam, fa, L, gx, gy); }                // A
        PT_CLK(0);
        {                                                                                                 // B
            const bool walking = L.stage == ST_WALKC;
            const Ray wr = lane_closest_ray<MEDIUM>(L);
            const RayPre p = ray_pre(wr);
            if (walking && L.fresh) { walk_begin(sc, false, wr, PT_INF, p, L.w, stk); L.fresh = false; }
            const bool go = walking && !L.w.done;
            const unsigned n_start = (unsigned)__popcll(__ballot(go));
            const unsigned n_other = (unsigned)__popcll(__ballot((walking && L.w.done) || L.stage == ST_BACK));
            if (go) {
                for (;;) {
                    if (!L.w.pend_count) walk_box(sc, false, wr, p, L.w, stk);
                    // the triangles that the box steps found are tested once enough of the walking lanes have one pending (or the
                    // phase is about to end: a pending lane tests at least one per iteration of the wave)
                    const bool pending = L.w.pend_count != 0u;
                    const unsigned n_in = (unsigned)__popcll(__ballot(1)), n_pend = (unsigned)__popcll(__ballot(pending));
                    const unsigned n_act = (unsigned)__popcll(__ballot(!L.w.done));
                    const bool cut = n_act < T && n_other + (n_start - n_act) > PT_WAIT_RATIO * n_act;   // the lanes that wait outnumber the walkers
                    if (pending && (n_pend * 16u >= n_in * TQ || cut)) walk_tri(sc, false, wr, L.w);
                    if (L.w.done || cut) break;
                }
            }
            PT_CLK(1);
            if (walking && L.w.done) { PT_WSTAT(5); lane_closest_done<MATS, MEDIUM>(sc, L); }
            PT_CLK(2);
        }
        if (L.stage == ST_BACK) { PT_WSTAT(6); lane_back<MATS, MEDIUM>(sc, L); }                         // C
        PT_CLK(3);
        {                                                                                                 // D
            const bool walking = L.stage == ST_WALKS;
            const Ray wr = lane_shadow_ray<MEDIUM, (MATS & PT_MATS_ENVIS) != 0>(L);
            const RayPre p = ray_pre(wr);
            if (walking && L.fresh) { walk_begin(sc, true, wr, wr.t, p, L.w, stk); L.fresh = false; }
            const bool go = walking && !L.w.done;
            const unsigned n_start = (unsigned)__popcll(__ballot(go));
            const unsigned n_other = (unsigned)__popcll(__ballot((walking && L.w.done) || L.stage == ST_FINISH));
            if (go) {
                for (;;) {
                    if (!L.w.pend_count) walk_box(sc, true, wr, p, L.w, stk);
                    const bool pending = L.w.pend_count != 0u;
                    const unsigned n_in = (unsigned)__popcll(__ballot(1)), n_pend = (unsigned)__popcll(__ballot(pending));
                    const unsigned n_act = (unsigned)__popcll(__ballot(!L.w.done));
                    const bool cut = n_act < TD && n_other + (n_start - n_act) > PT_WAIT_RATIO * n_act;
                    if (pending && (n_pend * 16u >= n_in * TQ || cut)) walk_tri(sc, true, wr, L.w);
                    if (L.w.done || cut) break;
                }
            }
            if (walking && L.w.done) { L.occluded = L.w.found; L.stage = ST_FINISH; }
        }
        PT_CLK(4);
        if (L.stage == ST_FINISH) { PT_WSTAT(7); lane_finish<MATS, MEDIUM>(sc, L); }                           // E
        PT_CLK(5);
#if PT_RK_ADAPT
        if (L.f != f_iter && L.reset) {
            // the segment ended the pixel's path: one 8-byte load and store per path (prt.h prt_render_adaptive)
            const float2 p = fa.adapt[id];
            const float lum = 0.2126f * L.acc[0] + 0.7152f * L.acc[1] + 0.0722f * L.acc[2];
            const float y = lum - p.x;
            const float s2 = p.y + y * y;
            fa.adapt[id] = make_float2(lum, s2);
            L.conv = L.samples >= fa.min_spp && adaptive_converged(lum, s2, L.samples, fa.rel_err, fa.abs_floor);
        }
#endif
#ifdef PT_PHASE_CLOCKS
        ++clk_[6];
#endif
    }
#ifdef PT_PHASE_CLOCKS
    if (lane == (int)__builtin_ctzll(__ballot(1))) {
        for (int k = 0; k < 8; ++k) atomicAdd(&g_phase_clocks[k], clk_[k]);
        atomicMax(&g_phase_clocks[8], clk_[6]);
        atomicMax(&g_phase_clocks[9], last_ - start_);
        atomicAdd(&g_phase_clocks[10], 1ull);
        atomicAdd(&g_phase_clocks[11], done_lanes_);
    }
#endif
    if (in_frame && L.f) {
        // frames of the NEXT launch already done (run_ahead); a frozen pixel owes nothing and is ahead of nothing
#if !PT_RK_ADAPT
        const bool frozen = fa.spp_limit && L.reset && L.samples >= fa.spp_limit;
#else
        const bool frozen = lane_frozen_adaptive(fa, L);
#endif
        const unsigned frames_ahead = (!frozen && L.f > fa.n_frames) ? L.f - fa.n_frames : 0u;
        S.q0[id] = make_float4(L.origin.x, L.origin.y, L.origin.z, L.t);
        S.q1[id] = make_float4(L.dir.x, L.dir.y, L.dir.z, L.time);
        S.q2[id] = make_float4(L.mask.x, L.mask.y, L.mask.z, prt_u2f(L.total));
        S.q3[id] = make_float4(L.acc[0], L.acc[1], L.acc[2], L.acc[3]);
#if !PT_RK_ADAPT
        S.q4[id] = make_uint4(L.samples, (L.diff & 0xffffu) | (L.spec << 16), (L.trans & 0xffffu) | (L.scatters << 16),
                              (L.wasSpecular ? 1u : 0u) | (L.reset ? 2u : 0u) | (frames_ahead << 2));
#else
        S.q4[id] = make_uint4(L.samples, (L.diff & 0xffffu) | (L.spec << 16), (L.trans & 0xffffu) | (L.scatters << 16),
                              (L.wasSpecular ? 1u : 0u) | (L.reset ? 2u : 0u) | (frames_ahead << 2) | (L.conv ? 0x80000000u : 0u));
#endif
        const float ns = (MATS & PT_MATS_VIEW) ? 1.0f : (float)L.samples;      // write_imagef, main.cl:159 (a debug view: :161)
        fb[id] = make_float4(L.acc[0] / ns, L.acc[1] / ns, L.acc[2] / ns, L.acc[3] / ns);
    }
    if (ORDER && !fa.scatter && fa.tile_cost && lane == 0) atomicMax(&fa.tile_cost[tile_k], iterations);     // (the longest of the tile's waves)
    if (fa.unfinished) {
#if !PT_RK_ADAPT
        const bool unfinished = in_frame && !(fa.spp_limit && L.reset && L.samples >= fa.spp_limit);
#else
        const bool unfinished = in_frame && !lane_frozen_adaptive(fa, L);
#endif
        const unsigned long long m = __ballot(unfinished);
        if (lane == (int)__builtin_ctzll(__ballot(1))) {
            // returning atomic: its value is back only once the add has been performed at the device's coherence point
            const unsigned long long before = m ? atomicAdd(fa.unfinished, (unsigned long long)__popcll(m)) : 0ull;
            if (fa.unfinished_host && before != ~0ull) {       // (never equal: the test orders the ticket behind the add without a
                // fence -- a device-scope fence writes back and invalidates this XCD's L2, 2.5 % when every wave does it)
                // The last wave of the launch hands the total to the host and leaves the counters clean for the next launch
                // (no wave returns early, so every wave of the grid gets here).
                if (atomicAdd(fa.unfinished + 1, 1ull) == (unsigned long long)gridDim.x - 1ull) {
                    const unsigned long long total = atomicExch(fa.unfinished, 0ull);
                    atomicExch(fa.unfinished + 1, 0ull);
                    *reinterpret_cast<volatile unsigned long long*>(fa.unfinished_host) = total;   // visible to the host at kernel end
                }
            }
        }
    }
