// tests/emu/refit_emu.cpp -- TEST INFRASTRUCTURE: the bodies of the refit kernels (csrc/hip/pt_refit.h) compiled for the host and run serially
// over pack_scene's output, in the order the device's launches impose: the check, every slot's records, then the pairs level by level,
// deepest first.  tests/emu/refit_api.py binds it.  With -DREFIT_EMU_MAIN a stand-alone program for sanitizer runs (see main below).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "prt.h"
#include "pt_pack.h"
#include "pt_refit.h"

using namespace prt;

struct RefitEmu {
    PackedScene ps;
    float root[6];
};

// what prt_update_vertices_device does, serially; 1 = refused (a non-finite vertex: nothing was written)
static int run_update(RefitEmu* h, uint32_t n_tris, const float* vertices, const float* normals) {
    PackedScene& ps = h->ps;
    for (size_t i = 0; i < 3 * (size_t)n_tris; ++i)
        if (!refit_vertex_finite(vertices, i)) return 1;
    for (size_t s = 0; s < ps.slot_vtx.size(); ++s) refit_tri(vertices, normals, ps.slot_vtx.data(), s, ps.tg.data(), ps.tn.data());
    if (ps.sc.root_is_leaf) {
        refit_root_leaf(vertices, ps.slot_vtx.data(), ps.sc.root_leaf_first, ps.sc.root_leaf_count, h->root);
        return 0;
    }
    for (size_t l = ps.level_first.size() - 1; l-- > 0;)
        for (uint32_t i = ps.level_first[l]; i < ps.level_first[l + 1]; ++i)
            refit_pair(ps.pairs.data(), ps.level_pairs[i], vertices, ps.slot_vtx.data(), h->root);
    return 0;
}

extern "C" {

int refit_emu_pack(const prt_config* cfg, const prt_scene_desc* desc, RefitEmu** out, char* err, int errlen) {
    RefitEmu* h = new RefitEmu();
    std::string e;
    const int rc = pack_scene(*cfg, desc, h->ps, e);
    if (rc) {
        if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", e.c_str());
        delete h;
        return rc;
    }
    std::memcpy(h->root, h->ps.root_bounds, sizeof(h->root));
    *out = h;
    return 0;
}

void refit_emu_free(RefitEmu* h) { delete h; }

// {pairs, slots, levels, nodes, root_is_leaf, stack_levels}
void refit_emu_sizes(const RefitEmu* h, uint32_t* out6) {
    out6[0] = (uint32_t)h->ps.pairs.size(); out6[1] = (uint32_t)h->ps.slot_vtx.size();
    out6[2] = h->ps.level_first.empty() ? 0u : (uint32_t)h->ps.level_first.size() - 1u;
    out6[3] = (uint32_t)h->ps.node_box.size(); out6[4] = (uint32_t)h->ps.sc.root_is_leaf; out6[5] = h->ps.sc.stack_levels;
}

// copies of the records and tables (any pointer may be null); root6: the root's box -- as uploaded, or of the last refit_emu_update
void refit_emu_get(const RefitEmu* h, void* pairs, void* tri_geom, void* tri_nrm, float* root6, uint32_t* slot_vtx, uint32_t* level_pairs,
                   uint32_t* level_first, uint32_t* node_box) {
    const PackedScene& ps = h->ps;
    if (pairs && !ps.pairs.empty()) std::memcpy(pairs, ps.pairs.data(), ps.pairs.size() * sizeof(NodePair));
    if (tri_geom && !ps.tg.empty()) std::memcpy(tri_geom, ps.tg.data(), ps.tg.size() * sizeof(TriGeom));
    if (tri_nrm && !ps.tn.empty()) std::memcpy(tri_nrm, ps.tn.data(), ps.tn.size() * sizeof(TriNrm));
    if (root6) std::memcpy(root6, h->root, sizeof(h->root));
    if (slot_vtx && !ps.slot_vtx.empty()) std::memcpy(slot_vtx, ps.slot_vtx.data(), ps.slot_vtx.size() * 4);
    if (level_pairs && !ps.level_pairs.empty()) std::memcpy(level_pairs, ps.level_pairs.data(), ps.level_pairs.size() * 4);
    if (level_first && !ps.level_first.empty()) std::memcpy(level_first, ps.level_first.data(), ps.level_first.size() * 4);
    if (node_box && !ps.node_box.empty()) std::memcpy(node_box, ps.node_box.data(), ps.node_box.size() * 4);
}

int refit_emu_update(RefitEmu* h, uint32_t n_tris, const float* vertices, const float* normals) { return run_update(h, n_tris, vertices, normals); }

}  // extern "C"

#ifdef REFIT_EMU_MAIN
// Sanitizer program (development, CPU only): built with the host model (csrc/host/*.cpp) and pt_pack.cpp under -fsanitize=address,undefined.
// Loads a scene file, deforms its mesh, runs the bodies, and checks the records against pack_scene's of the deformed vertices and every
// parent box against its children.  usage: refit_emu_main <scene.json> <models dir>
#include "host_capi.h"

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s scene.json models_dir\n", argv[0]); return 2; }
    char err[512] = "";
    prth_scene* sc = prth_scene_load(argv[1], argv[2], err, sizeof(err));
    if (!sc) { std::fprintf(stderr, "load: %s\n", err); return 2; }
    prt_scene_desc desc;
    prt_config cfg;
    prth_scene_get_desc(sc, &desc);
    prth_scene_get_config(sc, 0, &cfg);
    RefitEmu* h = nullptr;
    if (refit_emu_pack(&cfg, &desc, &h, err, sizeof(err))) { std::fprintf(stderr, "pack: %s\n", err); return 2; }
    const uint32_t T = desc.triangle_count;
    std::vector<float> v(desc.vertices, desc.vertices + 12 * (size_t)T), n(desc.normals, desc.normals + 12 * (size_t)T);
    for (size_t i = 0; i < 3 * (size_t)T; ++i) { v[4 * i + 1] *= 1.25f; v[4 * i] += 0.125f * v[4 * i + 1]; }
    if (run_update(h, T, v.data(), n.data())) { std::fprintf(stderr, "refused\n"); return 1; }
    prt_scene_desc d2 = desc;
    d2.vertices = v.data(); d2.normals = n.data();
    RefitEmu* g = nullptr;
    if (refit_emu_pack(&cfg, &d2, &g, err, sizeof(err))) { std::fprintf(stderr, "pack 2: %s\n", err); return 2; }
    int bad = 0;
    bad += std::memcmp(h->ps.tg.data(), g->ps.tg.data(), g->ps.tg.size() * sizeof(TriGeom)) != 0;
    bad += std::memcmp(h->ps.tn.data(), g->ps.tn.data(), g->ps.tn.size() * sizeof(TriNrm)) != 0;
    for (const NodePair& p : h->ps.pairs)
        for (int ch = 0; ch < 2; ++ch)
            if (p.meta[2 * ch + 1] == 0xFFFFFFFFu) {
                const NodePair& c = h->ps.pairs[p.meta[2 * ch]];
                for (int a = 0; a < 3; ++a) {
                    const float lo = c.b[2 * a] < c.b[6 + 2 * a] ? c.b[2 * a] : c.b[6 + 2 * a], hi = c.b[2 * a + 1] > c.b[7 + 2 * a] ? c.b[2 * a + 1] : c.b[7 + 2 * a];
                    bad += !(p.b[6 * ch + 2 * a] == lo && p.b[6 * ch + 2 * a + 1] == hi);
                }
            }
    // a refusal writes nothing
    v[5] = __builtin_nanf("");
    bad += run_update(h, T, v.data(), nullptr) != 1;
    std::printf("refit_emu_main: %u triangles, %zu pairs, %zu levels, %d mismatches\n", T, h->ps.pairs.size(), h->ps.level_first.empty() ? (size_t)0 : h->ps.level_first.size() - 1, bad);
    refit_emu_free(h); refit_emu_free(g);
    prth_scene_free(sc);
    return bad ? 1 : 0;
}
#endif
