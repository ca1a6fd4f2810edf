// pt_inst_filter_generic.hip -- render_kernel compiled for the material set generic under a pixel filter (PT_MATS_FILTER, prt_set_pixel_filter),
// medium off / on
#include "pt_render.h"

namespace prt {

PT_DECLARE_SET(launch_set_filter_generic) {
    constexpr unsigned M = PT_MATS_FILTER;
    if (medium) return launch_variant<M, true>("render_kernel<generic,medium,filter>", sc, cam, S, fa, fb, stream, lo);
    return launch_variant<M, false>("render_kernel<generic,filter>", sc, cam, S, fa, fb, stream, lo);
}

}  // namespace prt
