// pt_inst_filter_light_diff.hip -- render_kernel for the set LIGHT|DIFF under a pixel filter (prt_set_pixel_filter), medium off / on (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_FILTER_LIGHT_DIFF(PT_INSTANTIATE_VARIANT) }
