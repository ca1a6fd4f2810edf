// pt_inst_filter_rough_diel.hip -- render_kernel for the set LIGHT|DIFF|DIEL|ROUGH_DIEL under a pixel filter, GGX alone, without a medium (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_FILTER_ROUGH_DIEL(PT_INSTANTIATE_VARIANT) }
