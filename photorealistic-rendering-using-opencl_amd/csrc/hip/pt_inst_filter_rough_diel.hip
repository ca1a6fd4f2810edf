// pt_inst_filter_rough_diel.hip -- render_kernel compiled for the material set LIGHT|DIFF|DIEL|ROUGH_DIEL under a pixel filter (PT_MATS_FILTER,
// prt_set_pixel_filter), without a medium, for scenes whose microfacet lobes are all GGX (the build the unfiltered set takes for them; any other
// scene of the set, "any_dist" and a medium run the filtered generic dispatch)
#include "pt_render.h"

namespace prt {

PT_DECLARE_SET(launch_set_filter_rough_diel) {
    constexpr unsigned M = PRT_MAT_LIGHT | PRT_MAT_DIFF | PRT_MAT_DIEL | PRT_MAT_ROUGH_DIEL | PT_MATS_FILTER;
    if (medium || lo.any_dist || sc.dist_mask != (unsigned)PRT_DIST_GGX) return launch_set_filter_generic(medium, sc, cam, S, fa, fb, stream, lo);
    return launch_variant<M | ((unsigned)PRT_DIST_GGX << PT_MATS_DIST_SHIFT), false>("render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL; GGX,filter>", sc, cam, S, fa, fb, stream, lo);
}

}  // namespace prt
