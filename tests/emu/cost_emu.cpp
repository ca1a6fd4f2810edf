// tests/emu/cost_emu.cpp -- TEST INFRASTRUCTURE: the bodies of the tree-cost kernels (csrc/hip/pt_cost.h) compiled for the host and run serially
// over a pair table: every pair's term, then the pairwise tree level by level until one value is left, then the root's formula.  Two doors:
// the table of a packed scene (pack_scene's output, optionally refitted by the refit's bodies as refit_emu.cpp runs them), and a caller's
// table.  tests/emu/cost_api.py binds it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "prt.h"
#include "pt_cost.h"
#include "pt_pack.h"
#include "pt_refit.h"

using namespace prt;

struct CostEmu {
    PackedScene ps;
    float root[6];
};

// S of a table of n >= 1 pairs: cost_term per pair, then cost_level until one value is left
static double run_sum(const NodePair* pairs, size_t n) {
    std::vector<double> a(n), b;
    for (size_t k = 0; k < n; ++k) a[k] = cost_term(pairs, k);
    while (a.size() > 1) {
        b.assign((a.size() + 1) / 2, 0.0);
        for (size_t i = 0; i < b.size(); ++i) cost_level(a.data(), a.size(), b.data(), i);
        a.swap(b);
    }
    return a[0];
}

// out2 = {cost, S} (S = 0 for a leaf root)
static void run_cost(const NodePair* pairs, size_t n_pairs, const float* root6, int root_is_leaf, uint32_t leaf_count, double* out2) {
    if (root_is_leaf) { out2[0] = cost_leaf_root(root6, leaf_count); out2[1] = 0.0; return; }
    out2[1] = run_sum(pairs, n_pairs);
    out2[0] = cost_inner_root(pairs, out2[1]);
}

extern "C" {

int cost_emu_pack(const prt_config* cfg, const prt_scene_desc* desc, CostEmu** out, char* err, int errlen) {
    CostEmu* h = new CostEmu();
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

void cost_emu_free(CostEmu* h) { delete h; }

// {pairs, slots, levels, nodes, root_is_leaf, root_leaf_count}
void cost_emu_sizes(const CostEmu* h, uint32_t* out6) {
    out6[0] = (uint32_t)h->ps.pairs.size(); out6[1] = (uint32_t)h->ps.slot_vtx.size();
    out6[2] = h->ps.level_first.empty() ? 0u : (uint32_t)h->ps.level_first.size() - 1u;
    out6[3] = (uint32_t)h->ps.node_box.size(); out6[4] = (uint32_t)h->ps.sc.root_is_leaf; out6[5] = h->ps.sc.root_leaf_count;
}

// copies of the pair table and the root's box -- as uploaded, or of the last cost_emu_update (either pointer may be null)
void cost_emu_get(const CostEmu* h, void* pairs, float* root6) {
    if (pairs && !h->ps.pairs.empty()) std::memcpy(pairs, h->ps.pairs.data(), h->ps.pairs.size() * sizeof(NodePair));
    if (root6) std::memcpy(root6, h->root, sizeof(h->root));
}

// what prt_update_vertices_device does to the boxes, serially (refit_emu.cpp run_update); 1 = refused (a non-finite vertex)
int cost_emu_update(CostEmu* h, uint32_t n_tris, const float* vertices) {
    PackedScene& ps = h->ps;
    for (size_t i = 0; i < 3 * (size_t)n_tris; ++i)
        if (!refit_vertex_finite(vertices, i)) return 1;
    if (ps.sc.root_is_leaf) {
        refit_root_leaf(vertices, ps.slot_vtx.data(), ps.sc.root_leaf_first, ps.sc.root_leaf_count, h->root);
        return 0;
    }
    for (size_t l = ps.level_first.size() - 1; l-- > 0;)
        for (uint32_t i = ps.level_first[l]; i < ps.level_first[l + 1]; ++i)
            refit_pair(ps.pairs.data(), ps.level_pairs[i], vertices, ps.slot_vtx.data(), h->root);
    return 0;
}

// door 1: the packed scene's table as it is now
void cost_emu_cost(const CostEmu* h, double* out2) {
    run_cost(h->ps.pairs.data(), h->ps.pairs.size(), h->root, h->ps.sc.root_is_leaf, h->ps.sc.root_leaf_count, out2);
}

// door 2: a caller's table of n_pairs NodePair records (16-byte aligned) under an inner root, or -- root_is_leaf -- a leaf root of leaf_count
// triangles with the box root6
void cost_emu_table(const void* pairs, uint32_t n_pairs, const float* root6, int root_is_leaf, uint32_t leaf_count, double* out2) {
    run_cost(static_cast<const NodePair*>(pairs), n_pairs, root6, root_is_leaf, leaf_count, out2);
}

}  // extern "C"
