// pt_variant.h -- which builds of render_kernel exist, and which of them a launch takes.  Host only; ONE statement of the rule for the launcher
// (launch_render, pt_kernels.hip), the CPU emulator (tests/emu/pt_emu.cpp) and the tests of the rule itself (tests/test_variant_select.py).
//
// The builds are the AOT analogue of the reference's per-scene program build (include/CL/cl_kernel.h:226-345 compiles exactly the scene's
// ACTIVE_MATS): the material sets of the BASELINE configs are compiled -- LIGHT|DIFF, +COAT, +ROUGH_COND, +DIEL|ROUGH_DIEL -- and any other set
// runs the generic variant, which dispatches on the material's type bits at run time: the same code, the same bits.
//
// A new set or build axis is one row here and nothing else: the instance file named in the row's first column instantiates its group
// (PT_INSTANTIATE_VARIANT, pt_render.h), the launcher and the emulator dispatch over PT_VARIANTS.
#pragma once
#include "prt.h"
#include "prt_types.h"
#include "pt_launch.h"
#include "pt_layout.h"

namespace prt {

#define PT_SET_LIGHT_DIFF (PRT_MAT_LIGHT | PRT_MAT_DIFF)                                           // configs 2, 4, 5: Lambert + light
#define PT_SET_COAT (PRT_MAT_LIGHT | PRT_MAT_DIFF | PRT_MAT_COAT)                                  // config 1 (scenes/cornell.json as shipped)
#define PT_SET_ROUGH_COND (PRT_MAT_LIGHT | PRT_MAT_DIFF | PRT_MAT_ROUGH_COND)                      // config 3a
#define PT_SET_ROUGH_DIEL (PRT_MAT_LIGHT | PRT_MAT_DIFF | PRT_MAT_DIEL | PRT_MAT_ROUGH_DIEL)       // config 3b
#define PT_MATS_BECKMANN ((unsigned)PRT_DIST_BECKMANN << PT_MATS_DIST_SHIFT)                       // PT_MATS_DISTS: every microfacet lobe of the scene is ...
#define PT_MATS_GGX ((unsigned)PRT_DIST_GGX << PT_MATS_DIST_SHIFT)

// ---- the table: X(instance file pt_inst_<file>.hip, MATS, MEDIUM, prt_kernel_variant's name), grouped by the file that compiles the row.
// The coat, rough conductor and rough dielectric sets are not compiled with a medium (no BASELINE config has both); each is compiled once more
// for the one distribution its BASELINE config uses, and under a pixel filter (PT_MATS_FILTER) for that distribution only.
#define PT_VARIANTS_LIGHT_DIFF(X) \
    X(light_diff, PT_SET_LIGHT_DIFF, false, "render_kernel<LIGHT|DIFF>") \
    X(light_diff, PT_SET_LIGHT_DIFF, true, "render_kernel<LIGHT|DIFF,medium>")
#define PT_VARIANTS_COAT(X) \
    X(coat, PT_SET_COAT, false, "render_kernel<LIGHT|DIFF|COAT>") \
    X(coat, PT_SET_COAT | PT_MATS_BECKMANN, false, "render_kernel<LIGHT|DIFF|COAT; Beckmann>")
#define PT_VARIANTS_ROUGH_COND(X) \
    X(rough_cond, PT_SET_ROUGH_COND, false, "render_kernel<LIGHT|DIFF|ROUGH_COND>") \
    X(rough_cond, PT_SET_ROUGH_COND | PT_MATS_GGX, false, "render_kernel<LIGHT|DIFF|ROUGH_COND; GGX>")
#define PT_VARIANTS_ROUGH_DIEL(X) \
    X(rough_diel, PT_SET_ROUGH_DIEL, false, "render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL>") \
    X(rough_diel, PT_SET_ROUGH_DIEL | PT_MATS_GGX, false, "render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL; GGX>")
#define PT_VARIANTS_GENERIC(X) \
    X(generic, 0u, false, "render_kernel<generic>") \
    X(generic, 0u, true, "render_kernel<generic,medium>")
#define PT_VARIANTS_SDF(X)          /* H_SDF scenes: the generic set with the raymarcher */ \
    X(sdf, PT_MATS_SDF, false, "render_kernel<generic,sdf>") \
    X(sdf, PT_MATS_SDF, true, "render_kernel<generic,sdf,medium>")
#define PT_VARIANTS_VIEW(X)         /* the debug views VIEW_NORMAL / VIEW_BVH_HIT */ \
    X(view, PT_MATS_VIEW, false, "render_kernel<generic,view>") \
    X(view, PT_MATS_VIEW, true, "render_kernel<generic,view,medium>")
#define PT_VARIANTS_VIEW_SDF(X) \
    X(view_sdf, PT_MATS_VIEW | PT_MATS_SDF, false, "render_kernel<generic,sdf,view>") \
    X(view_sdf, PT_MATS_VIEW | PT_MATS_SDF, true, "render_kernel<generic,sdf,view,medium>")
#define PT_VARIANTS_PICK(X)         /* PICK_RANDOM_LIGHT (kernels/integrators/base.cl:9) */ \
    X(pick, PT_MATS_PICK, false, "render_kernel<generic,pick_random_light>") \
    X(pick, PT_MATS_PICK, true, "render_kernel<generic,pick_random_light,medium>")
#define PT_VARIANTS_ENVIS(X)        /* environment-map importance sampling (not in the reference): surfaces only */ \
    X(envis, PT_MATS_ENVIS, false, "render_kernel<generic,env_importance_sampling>")
#define PT_VARIANTS_FILTER_LIGHT_DIFF(X) \
    X(filter_light_diff, PT_SET_LIGHT_DIFF | PT_MATS_FILTER, false, "render_kernel<LIGHT|DIFF,filter>") \
    X(filter_light_diff, PT_SET_LIGHT_DIFF | PT_MATS_FILTER, true, "render_kernel<LIGHT|DIFF,medium,filter>")
#define PT_VARIANTS_FILTER_COAT(X) \
    X(filter_coat, PT_SET_COAT | PT_MATS_BECKMANN | PT_MATS_FILTER, false, "render_kernel<LIGHT|DIFF|COAT; Beckmann,filter>")
#define PT_VARIANTS_FILTER_ROUGH_COND(X) \
    X(filter_rough_cond, PT_SET_ROUGH_COND | PT_MATS_GGX | PT_MATS_FILTER, false, "render_kernel<LIGHT|DIFF|ROUGH_COND; GGX,filter>")
#define PT_VARIANTS_FILTER_ROUGH_DIEL(X) \
    X(filter_rough_diel, PT_SET_ROUGH_DIEL | PT_MATS_GGX | PT_MATS_FILTER, false, "render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL; GGX,filter>")
#define PT_VARIANTS_FILTER_GENERIC(X) \
    X(filter_generic, PT_MATS_FILTER, false, "render_kernel<generic,filter>") \
    X(filter_generic, PT_MATS_FILTER, true, "render_kernel<generic,medium,filter>")

#ifdef PT_DEV_ONE_VARIANT           // development builds (tools/): only the headline set, compiles in seconds
#define PT_VARIANTS(X) PT_VARIANTS_LIGHT_DIFF(X)
#else
#define PT_VARIANTS(X) \
    PT_VARIANTS_LIGHT_DIFF(X) PT_VARIANTS_COAT(X) PT_VARIANTS_ROUGH_COND(X) PT_VARIANTS_ROUGH_DIEL(X) PT_VARIANTS_GENERIC(X) \
    PT_VARIANTS_SDF(X) PT_VARIANTS_VIEW(X) PT_VARIANTS_VIEW_SDF(X) PT_VARIANTS_PICK(X) PT_VARIANTS_ENVIS(X) \
    PT_VARIANTS_FILTER_LIGHT_DIFF(X) PT_VARIANTS_FILTER_COAT(X) PT_VARIANTS_FILTER_ROUGH_COND(X) PT_VARIANTS_FILTER_ROUGH_DIEL(X) \
    PT_VARIANTS_FILTER_GENERIC(X)
#endif

struct Variant { unsigned mats; bool medium; const char* name; const char* file; };
#define PT_VARIANT_ROW(file, M, MED, name) {(M), (MED), name, "pt_inst_" #file ".hip"},
inline constexpr Variant k_variants[] = {PT_VARIANTS(PT_VARIANT_ROW)};
inline constexpr int k_n_variants = (int)(sizeof(k_variants) / sizeof(k_variants[0]));

// what of a packed scene (DevScene) and a launch (FrameArgs::filter_kind) the choice depends on
struct VariantKey {
    unsigned active_mats, dist_mask, n_sdfs, filter_kind;
    bool has_medium, view, pick_random_light, env_is;
};

// the scene's own material set (with its PT_MATS_DISTS bits) where it is compiled, else 0: the run-time dispatch
inline unsigned compiled_set(const VariantKey& k, const LaunchOpts& lo, bool filter) {
    const unsigned am = k.active_mats;
    if (lo.generic) return 0u;                              // LaunchOpts::generic forces the dispatch: the tests run every golden through both
    if (am == PT_SET_LIGHT_DIFF) return am;                 // no microfacet lobe; medium off / on, filtered or not
    if (k.has_medium || !(am == PT_SET_COAT || am == PT_SET_ROUGH_COND || am == PT_SET_ROUGH_DIEL)) return 0u;
    const unsigned dist = am == PT_SET_COAT ? (unsigned)PRT_DIST_BECKMANN : (unsigned)PRT_DIST_GGX;     // of the set's BASELINE config
    if (!lo.any_dist && k.dist_mask == dist) return am | (dist << PT_MATS_DIST_SHIFT);
    return filter ? 0u : am;                                // every distribution: not compiled under a filter
}

// The row a launch takes (null if the table lacked it: every key has a row, tests/test_variant_select.py enumerates them).
// pack_scene refuses env sampling with a medium, SDFs, views or the light pick, and the light pick with SDFs or views; prt_set_pixel_filter
// refuses what filter_unsupported names -- so each branch sees only the flags it reads.
inline const Variant* select_variant(const VariantKey& k, const LaunchOpts& lo) {
    bool medium = k.has_medium;
    unsigned mats;
    if (k.filter_kind != PRT_FILTER_NONE) mats = compiled_set(k, lo, true) | PT_MATS_FILTER;
    else if (k.env_is) { mats = PT_MATS_ENVIS; medium = false; }
    else if (k.pick_random_light) mats = PT_MATS_PICK;
    else if (k.view) mats = PT_MATS_VIEW | (k.n_sdfs ? PT_MATS_SDF : 0u);
    else if (k.n_sdfs) mats = PT_MATS_SDF;
    else mats = compiled_set(k, lo, false);
    for (const Variant& v : k_variants)
        if (v.mats == mats && v.medium == medium) return &v;
    return nullptr;
}

// why prt_set_pixel_filter refuses a config (no PT_MATS_FILTER rows of these sets), or null
inline const char* filter_unsupported(const prt_config& cfg) {
    return cfg.view_option != PRT_VIEW_RESULTS ? "a debug view" : (cfg.geom_flags & PRT_GEOM_SDF) ? "SDF primitives"
         : cfg.pick_random_light ? "pick_random_light" : cfg.env_importance_sampling ? "env_importance_sampling" : nullptr;
}

}  // namespace prt
