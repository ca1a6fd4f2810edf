// tests/emu/build_emu.cpp -- TEST INFRASTRUCTURE: the bodies of the build kernels (csrc/hip/pt_build.h) and of the refit kernels (pt_refit.h)
// compiled for the host and run serially over pack_scene's output, in the order the device's launches impose, with std::sort / a running sum
// where the device calls the library's sorts and scan, and with the bookkeeping of prt_rebuild_bvh_device (csrc/hip/prt_api_scene.cpp) around them:
// build into fresh tables, swap at the end, carry the normals and the motion snapshot.  tests/emu/build_api.py binds it.  With
// -DBUILD_EMU_MAIN a stand-alone program for sanitizer runs (see main below).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "prt.h"
#include "pt_build.h"
#include "pt_pack.h"
#include "pt_refit.h"

using namespace prt;

struct BuildEmu {
    PackedScene ps;                  // pairs, tg, tn, slot_vtx, level_pairs, level_first, sc.{n_pairs, stack_levels, root_*}: the current tree
    float root[6];
    uint32_t n_tris = 0;
    bool motion = false, snap_valid = false;
    std::vector<TriGeom> prev;       // the motion snapshot (slot order of the tree it was taken in, or the new one after a rebuild)
};

static void run_refit(PackedScene& ps, float* root, const float* vertices, const float* normals) {
    for (size_t s = 0; s < ps.slot_vtx.size(); ++s) refit_tri(vertices, normals, ps.slot_vtx.data(), s, ps.tg.data(), ps.tn.data());
    if (ps.sc.root_is_leaf) { refit_root_leaf(vertices, ps.slot_vtx.data(), ps.sc.root_leaf_first, ps.sc.root_leaf_count, root); return; }
    for (size_t l = ps.level_first.size() - 1; l-- > 0;)
        for (uint32_t i = ps.level_first[l]; i < ps.level_first[l + 1]; ++i) refit_pair(ps.pairs.data(), ps.level_pairs[i], vertices, ps.slot_vtx.data(), root);
}

// prt_update_vertices_device, serially; 1 = refused
static int run_update(BuildEmu* h, const float* vertices, const float* normals) {
    for (size_t i = 0; i < 3 * (size_t)h->n_tris; ++i)
        if (!refit_vertex_finite(vertices, i)) return 1;
    if (h->motion && !h->snap_valid) { h->prev = h->ps.tg; h->snap_valid = true; }
    run_refit(h->ps, h->root, vertices, normals);
    return 0;
}

// prt_rebuild_bvh_device, serially; 0, or 1 = a non-finite vertex, 2 = normals null and a triangle without a normal record, 3 = max_leaf
static int run_rebuild(BuildEmu* h, const float* vertices, const float* normals, uint32_t max_leaf) {
    if (max_leaf > 64u) return 3;
    if (!max_leaf) max_leaf = PT_BUILD_DEFAULT_LEAF;
    const uint32_t T = h->n_tris;
    PackedScene& ps = h->ps;
    for (size_t i = 0; i < 3 * (size_t)T; ++i)
        if (!refit_vertex_finite(vertices, i)) return 1;
    const bool carry_nrm = normals == nullptr, need_old = carry_nrm || h->motion;
    std::vector<uint32_t> old_slot(T, PT_BUILD_NONE);
    if (need_old) {
        for (uint32_t s = 0; s < ps.slot_vtx.size(); ++s) build_old_slot(ps.slot_vtx.data(), s, old_slot.data());
        if (carry_nrm)
            for (uint32_t i = 0; i < T; ++i)
                if (old_slot[i] == PT_BUILD_NONE) return 2;
    }
    // stages 1 and 2: block partials of 256 triangles, then one merge over them, as the device reduces
    const uint32_t parts = (T + 255u) / 256u;
    std::vector<float> partials(6 * (size_t)parts);
    for (uint32_t p = 0; p < parts; ++p) {
        float lo[3], hi[3];
        for (uint32_t i = 256u * p; i < 256u * p + 256u; ++i) {
            float c[3];
            build_centre(vertices, i < T ? i : T - 1u, c);
            if (i == 256u * p) for (int k = 0; k < 3; ++k) lo[k] = hi[k] = c[k];
            else build_extent_merge(lo, hi, c, c);
        }
        for (int k = 0; k < 3; ++k) { partials[6 * (size_t)p + k] = lo[k]; partials[6 * (size_t)p + 3 + k] = hi[k]; }
    }
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = partials[k]; hi[k] = partials[3 + k]; }
    for (uint32_t p = 1; p < parts; ++p) build_extent_merge(lo, hi, partials.data() + 6 * (size_t)p, partials.data() + 6 * (size_t)p + 3);
    const BuildExtent e = build_extent_finish(lo, hi);
    std::vector<uint64_t> keys(T);
    for (uint32_t i = 0; i < T; ++i) keys[i] = build_key(vertices, i, e);
    std::sort(keys.begin(), keys.end());
    // the new tables
    PackedScene nt;
    float new_root[6] = {0, 0, 0, 0, 0, 0};
    nt.slot_vtx.assign(T, 0u);
    nt.tg.assign(T, TriGeom{});
    nt.tn.assign(T, TriNrm{});
    nt.sc = ps.sc;
    const bool leaf_root = T <= max_leaf;
    if (leaf_root) {
        for (uint32_t s = 0; s < T; ++s) build_root_slot(keys.data(), s, nt.slot_vtx.data());
        nt.sc.n_pairs = 0; nt.sc.stack_levels = 1; nt.sc.root_is_leaf = 1; nt.sc.root_leaf_first = 0; nt.sc.root_leaf_count = T;
    } else {
        const uint32_t n = T - 1u;
        std::vector<BuildNode> nodes(n);
        std::vector<uint32_t> parent(n, 0u);
        for (uint32_t i = 0; i < n; ++i) build_node(keys.data(), T, i, nodes.data(), parent.data());
        BuildHeader hdr;
        std::memset(&hdr, 0, sizeof(hdr));
        std::vector<std::pair<uint64_t, uint32_t>> kv(n);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t two;
            kv[i] = {build_pair_key(nodes.data(), parent.data(), i, max_leaf, &two), i};
            if (two > hdr.max_two) hdr.max_two = two;
        }
        std::stable_sort(kv.begin(), kv.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first < b.first; });
        std::vector<uint64_t> pk(n);
        std::vector<uint32_t> order(n), pair_of(n, PT_BUILD_NONE), leaf_tris(n, 0u), slot_base(n, 0u);
        for (uint32_t k = 0; k < n; ++k) { pk[k] = kv[k].first; order[k] = kv[k].second; }
        for (uint32_t k = 0; k < n; ++k) build_number(pk.data(), order.data(), n, k, nodes.data(), max_leaf, pair_of.data(), leaf_tris.data(), &hdr);
        uint32_t run = 0;
        for (uint32_t k = 0; k < n; ++k) { slot_base[k] = run; run += leaf_tris[k]; }
        if (run != T || hdr.n_pairs == 0 || hdr.n_pairs > n || hdr.level_first[hdr.n_levels] != hdr.n_pairs) return 100;       // (a bug in the bodies)
        nt.pairs.assign(hdr.n_pairs, NodePair{});
        nt.level_pairs.assign(hdr.n_pairs, 0u);
        // (the device runs a lane per position; positions past the pairs return at once, and the tables here end with the pairs)
        for (uint32_t k = 0; k < hdr.n_pairs; ++k)
            build_pair(pk.data(), order.data(), k, nodes.data(), pair_of.data(), slot_base.data(), keys.data(), max_leaf, nt.pairs.data(), nt.slot_vtx.data(),
                       nt.level_pairs.data());
        for (uint32_t k = hdr.n_pairs; k < n; ++k)
            if ((uint32_t)(pk[k] >> 32) < PT_BUILD_NO_DEPTH) return 101;
        nt.level_first.assign(hdr.level_first, hdr.level_first + hdr.n_levels + 1u);
        nt.sc.n_pairs = hdr.n_pairs; nt.sc.stack_levels = hdr.max_two + 1u; nt.sc.root_is_leaf = 0; nt.sc.root_leaf_first = 0; nt.sc.root_leaf_count = 0;
    }
    run_refit(nt, new_root, vertices, normals);
    std::vector<TriGeom> new_prev;
    if (h->motion) new_prev.assign(T, TriGeom{});
    if (need_old) {
        const TriGeom* prev_old = h->snap_valid ? h->prev.data() : ps.tg.data();
        for (uint32_t s = 0; s < T; ++s)
            build_carry(nt.slot_vtx.data(), s, old_slot.data(), carry_nrm, ps.tn.data(), nt.tn.data(), prev_old, nt.tg.data(), h->motion ? new_prev.data() : nullptr);
    }
    // the swap
    ps.pairs.swap(nt.pairs); ps.tg.swap(nt.tg); ps.tn.swap(nt.tn); ps.slot_vtx.swap(nt.slot_vtx); ps.level_pairs.swap(nt.level_pairs);
    ps.level_first.swap(nt.level_first);
    ps.sc = nt.sc;
    ps.node_box.assign(2 * (size_t)ps.sc.n_pairs + 1, 0u);
    ps.node_box[0] = 0xFFFFFFFFu;
    for (size_t i = 1; i < ps.node_box.size(); ++i) ps.node_box[i] = (uint32_t)(i - 1);
    std::memcpy(h->root, new_root, sizeof(new_root));
    if (h->motion) { h->prev.swap(new_prev); h->snap_valid = true; }
    return 0;
}

// prt_read_bvh of a rebuilt tree, from the tables (rules 6 and 7)
static uint32_t read_tree(const BuildEmu* h, prt_bvh_node* nodes, uint64_t* prims) {
    const PackedScene& ps = h->ps;
    const uint32_t N = 2u * ps.sc.n_pairs + 1u;
    if (prims) for (size_t s = 0; s < ps.slot_vtx.size(); ++s) prims[s] = ps.slot_vtx[s] / 3u;
    if (!nodes) return N;
    std::memset(nodes, 0, sizeof(prt_bvh_node) * (size_t)N);
    std::memcpy(nodes[0].bounds, h->root, sizeof(h->root));
    if (ps.sc.root_is_leaf) {
        nodes[0].first_child_or_primitive = ps.sc.root_leaf_first; nodes[0].primitive_count = ps.sc.root_leaf_count; nodes[0].is_leaf = 1;
        return N;
    }
    nodes[0].first_child_or_primitive = 1;
    for (uint32_t k = 0; k < ps.sc.n_pairs; ++k)
        for (uint32_t ch = 0; ch < 2; ++ch) {
            prt_bvh_node& nd = nodes[2 * k + 1 + ch];
            std::memcpy(nd.bounds, ps.pairs[k].b + 6 * ch, 6 * sizeof(float));
            if (ps.pairs[k].meta[2 * ch + 1] == 0xFFFFFFFFu) nd.first_child_or_primitive = 2u * ps.pairs[k].meta[2 * ch] + 1u;
            else { nd.first_child_or_primitive = ps.pairs[k].meta[2 * ch]; nd.primitive_count = ps.pairs[k].meta[2 * ch + 1]; nd.is_leaf = 1; }
        }
    return N;
}

extern "C" {

int build_emu_pack(const prt_config* cfg, const prt_scene_desc* desc, BuildEmu** out, char* err, int errlen) {
    BuildEmu* h = new BuildEmu();
    std::string e;
    const int rc = pack_scene(*cfg, desc, h->ps, e);
    if (rc) {
        if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", e.c_str());
        delete h;
        return rc;
    }
    std::memcpy(h->root, h->ps.root_bounds, sizeof(h->root));
    h->n_tris = desc->triangle_count;
    *out = h;
    return 0;
}

void build_emu_free(BuildEmu* h) { delete h; }

// {pairs, slots, levels, nodes, root_is_leaf, stack_levels, root_leaf_first, root_leaf_count, snapshot pending, snapshot slots}
void build_emu_sizes(const BuildEmu* h, uint32_t* out10) {
    const PackedScene& ps = h->ps;
    out10[0] = (uint32_t)ps.pairs.size(); out10[1] = (uint32_t)ps.slot_vtx.size();
    out10[2] = ps.level_first.empty() ? 0u : (uint32_t)ps.level_first.size() - 1u;
    out10[3] = (uint32_t)ps.node_box.size(); out10[4] = (uint32_t)ps.sc.root_is_leaf; out10[5] = ps.sc.stack_levels;
    out10[6] = ps.sc.root_leaf_first; out10[7] = ps.sc.root_leaf_count; out10[8] = h->snap_valid ? 1u : 0u; out10[9] = (uint32_t)h->prev.size();
}

void build_emu_get(const BuildEmu* h, void* pairs, void* tri_geom, void* tri_nrm, float* root6, uint32_t* slot_vtx, uint32_t* level_pairs,
                   uint32_t* level_first, uint32_t* node_box, void* prev) {
    const PackedScene& ps = h->ps;
    if (pairs && !ps.pairs.empty()) std::memcpy(pairs, ps.pairs.data(), ps.pairs.size() * sizeof(NodePair));
    if (tri_geom && !ps.tg.empty()) std::memcpy(tri_geom, ps.tg.data(), ps.tg.size() * sizeof(TriGeom));
    if (tri_nrm && !ps.tn.empty()) std::memcpy(tri_nrm, ps.tn.data(), ps.tn.size() * sizeof(TriNrm));
    if (root6) std::memcpy(root6, h->root, sizeof(h->root));
    if (slot_vtx && !ps.slot_vtx.empty()) std::memcpy(slot_vtx, ps.slot_vtx.data(), ps.slot_vtx.size() * 4);
    if (level_pairs && !ps.level_pairs.empty()) std::memcpy(level_pairs, ps.level_pairs.data(), ps.level_pairs.size() * 4);
    if (level_first && !ps.level_first.empty()) std::memcpy(level_first, ps.level_first.data(), ps.level_first.size() * 4);
    if (node_box && !ps.node_box.empty()) std::memcpy(node_box, ps.node_box.data(), ps.node_box.size() * 4);
    if (prev && !h->prev.empty()) std::memcpy(prev, h->prev.data(), h->prev.size() * sizeof(TriGeom));
}

void build_emu_set_motion(BuildEmu* h, int on) { h->motion = on != 0; if (!on) { h->prev.clear(); h->snap_valid = false; } }
// what prt_render_guides does to the snapshot: consumed
void build_emu_consume_snapshot(BuildEmu* h) { h->snap_valid = false; }
int build_emu_update(BuildEmu* h, const float* vertices, const float* normals) { return run_update(h, vertices, normals); }
int build_emu_rebuild(BuildEmu* h, const float* vertices, const float* normals, uint32_t max_leaf) { return run_rebuild(h, vertices, normals, max_leaf); }
uint32_t build_emu_read_bvh(const BuildEmu* h, prt_bvh_node* nodes, uint64_t* prims) { return read_tree(h, nodes, prims); }

}  // extern "C"

#ifdef BUILD_EMU_MAIN
// Sanitizer program (development, CPU only): built with the host model (csrc/host/*.cpp) and pt_pack.cpp under -fsanitize=address,undefined.
// Loads a scene file, rebuilds its mesh's tree at several leaf sizes -- deformed, with and without normals, with motion on --, then the
// degenerate soups (one triangle, identical triangles, a planar sheet, two far clusters) under a leaf-root upload, and checks every result
// against pack_scene of the read-back tree.  usage: build_emu_main <scene.json> <models dir>
#include "host_capi.h"

static int check(BuildEmu* h, const prt_config& cfg, const prt_scene_desc& desc, const float* v, const float* n) {
    std::vector<prt_bvh_node> nodes(read_tree(h, nullptr, nullptr));
    std::vector<uint64_t> prims(desc.triangle_count);
    read_tree(h, nodes.data(), prims.data());
    prt_scene_desc d = desc;
    d.vertices = v; d.normals = n; d.bvh_nodes = nodes.data(); d.bvh_node_count = (uint32_t)nodes.size(); d.primitive_indices = prims.data();
    PackedScene want;
    std::string e;
    setenv("PRT_PAIR_ORDER", "bfs", 1);
    if (pack_scene(cfg, &d, want, e)) { std::fprintf(stderr, "pack of the read-back tree: %s\n", e.c_str()); return 1; }
    const PackedScene& g = h->ps;
    int bad = 0;
    bad += g.pairs.size() != want.pairs.size() || (!g.pairs.empty() && std::memcmp(g.pairs.data(), want.pairs.data(), g.pairs.size() * sizeof(NodePair)) != 0);
    bad += g.tg.size() != want.tg.size() || std::memcmp(g.tg.data(), want.tg.data(), g.tg.size() * sizeof(TriGeom)) != 0;
    bad += g.tn.size() != want.tn.size() || std::memcmp(g.tn.data(), want.tn.data(), g.tn.size() * sizeof(TriNrm)) != 0;
    bad += g.slot_vtx != want.slot_vtx; bad += g.level_pairs != want.level_pairs; bad += g.level_first != want.level_first;
    bad += g.sc.stack_levels != want.sc.stack_levels || g.sc.n_pairs != want.sc.n_pairs || g.sc.root_is_leaf != want.sc.root_is_leaf;
    bad += g.sc.root_leaf_first != want.sc.root_leaf_first || g.sc.root_leaf_count != want.sc.root_leaf_count;
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s scene.json models_dir\n", argv[0]); return 2; }
    char err[512] = "";
    prth_scene* sc = prth_scene_load(argv[1], argv[2], err, sizeof(err));
    if (!sc) { std::fprintf(stderr, "load: %s\n", err); return 2; }
    prt_scene_desc desc;
    prt_config cfg;
    prth_scene_get_desc(sc, &desc);
    prth_scene_get_config(sc, 0, &cfg);
    int bad = 0;
    const uint32_t T = desc.triangle_count;
    std::vector<float> v(desc.vertices, desc.vertices + 12 * (size_t)T), n(desc.normals, desc.normals + 12 * (size_t)T);
    for (size_t i = 0; i < 3 * (size_t)T; ++i) { v[4 * i + 1] *= 1.25f; v[4 * i] += 0.125f * v[4 * i + 1]; }
    const uint32_t leaves[] = {1u, 2u, 4u, 16u, 64u, 0u};
    for (uint32_t ml : leaves) {
        BuildEmu* h = nullptr;
        if (build_emu_pack(&cfg, &desc, &h, err, sizeof(err))) { std::fprintf(stderr, "pack: %s\n", err); return 2; }
        build_emu_set_motion(h, 1);
        bad += run_rebuild(h, v.data(), n.data(), ml) != 0;
        bad += check(h, cfg, desc, v.data(), n.data());
        bad += run_update(h, desc.vertices, nullptr) != 0;                    // a refit of the new topology, the normals kept
        bad += check(h, cfg, desc, desc.vertices, n.data());
        bad += run_rebuild(h, v.data(), nullptr, ml) != 0;                     // a rebuild of a rebuilt tree, the normals carried
        bad += check(h, cfg, desc, v.data(), n.data());
        v[5] = __builtin_nanf("");
        bad += run_rebuild(h, v.data(), nullptr, ml) != 1;                     // refusals write nothing
        v[5] = 0.25f;
        bad += run_rebuild(h, v.data(), nullptr, 65u) != 3;
        std::printf("build_emu_main: max_leaf %u: %u triangles, %zu pairs, %zu levels, %u stack levels\n", ml, T, h->ps.pairs.size(),
                    h->ps.level_first.empty() ? (size_t)0 : h->ps.level_first.size() - 1, h->ps.sc.stack_levels);
        build_emu_free(h);
    }
    // the soups, under a leaf root that names every triangle
    struct Soup { const char* name; uint32_t T; int kind; };
    const Soup soups[] = {{"one", 1, 0}, {"identical", 5, 1}, {"planar", 64, 2}, {"clusters", 40, 3}, {"ragged", 257, 0}};
    for (const Soup& sp : soups) {
        std::vector<float> sv(12 * (size_t)sp.T, 0.0f), sn(12 * (size_t)sp.T, 0.0f);
        uint32_t seed = 12345u;
        auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) * (1.0f / 16777216.0f); };
        for (uint32_t t = 0; t < sp.T; ++t)
            for (int k = 0; k < 3; ++k) {
                float* p = sv.data() + 4 * (3 * (size_t)t + k);
                if (sp.kind == 1) { p[0] = k == 1 ? 1.0f : 0.0f; p[1] = k == 2 ? 1.0f : 0.0f; p[2] = 0.5f; }
                else {
                    p[0] = rnd(); p[1] = rnd(); p[2] = sp.kind == 2 ? 0.25f : rnd();
                    if (sp.kind == 3) p[0] = (t & 1u) ? 100.0f + 0.001f * (float)k : -100.0f - 0.001f * (float)k;
                }
                sn[4 * (3 * (size_t)t + k) + 1] = 1.0f;
            }
        std::vector<uint64_t> prims(sp.T);
        for (uint32_t t = 0; t < sp.T; ++t) prims[t] = t;
        prt_bvh_node rootn;
        std::memset(&rootn, 0, sizeof(rootn));
        rootn.primitive_count = sp.T; rootn.is_leaf = 1;
        prt_scene_desc d = desc;
        d.vertices = sv.data(); d.normals = sn.data(); d.primitive_indices = prims.data(); d.triangle_count = sp.T; d.bvh_nodes = &rootn; d.bvh_node_count = 1;
        for (uint32_t ml : {1u, 4u, 64u}) {
            BuildEmu* h = nullptr;
            if (build_emu_pack(&cfg, &d, &h, err, sizeof(err))) { std::fprintf(stderr, "pack soup: %s\n", err); return 2; }
            bad += run_rebuild(h, sv.data(), nullptr, ml) != 0;
            bad += check(h, cfg, d, sv.data(), sn.data());
            std::printf("build_emu_main: soup %s, max_leaf %u: %zu pairs, %u stack levels\n", sp.name, ml, h->ps.pairs.size(), h->ps.sc.stack_levels);
            build_emu_free(h);
        }
    }
    std::printf("build_emu_main: %d mismatches\n", bad);
    prth_scene_free(sc);
    return bad ? 1 : 0;
}
#endif
