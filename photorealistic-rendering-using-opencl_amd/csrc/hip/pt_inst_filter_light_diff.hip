// pt_inst_filter_light_diff.hip -- render_kernel compiled for the material set LIGHT|DIFF under a pixel filter (PT_MATS_FILTER, prt_set_pixel_filter),
// medium off / on
#include "pt_render.h"

namespace prt {

PT_DECLARE_SET(launch_set_filter_light_diff) {
    constexpr unsigned M = PRT_MAT_LIGHT | PRT_MAT_DIFF | PT_MATS_FILTER;
    if (medium) return launch_variant<M, true>("render_kernel<LIGHT|DIFF,medium,filter>", sc, cam, S, fa, fb, stream, lo);
    return launch_variant<M, false>("render_kernel<LIGHT|DIFF,filter>", sc, cam, S, fa, fb, stream, lo);
}

}  // namespace prt
