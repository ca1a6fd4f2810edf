// pt_inst_filter_coat.hip -- render_kernel for the set LIGHT|DIFF|COAT under a pixel filter, Beckmann alone, without a medium (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_FILTER_COAT(PT_INSTANTIATE_VARIANT) }
