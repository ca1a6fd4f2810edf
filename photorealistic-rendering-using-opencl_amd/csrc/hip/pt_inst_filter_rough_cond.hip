// pt_inst_filter_rough_cond.hip -- render_kernel for the set LIGHT|DIFF|ROUGH_COND under a pixel filter, GGX alone, without a medium (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_FILTER_ROUGH_COND(PT_INSTANTIATE_VARIANT) }
