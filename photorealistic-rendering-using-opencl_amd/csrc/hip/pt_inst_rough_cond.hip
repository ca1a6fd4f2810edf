// pt_inst_rough_cond.hip -- render_kernel for the material set LIGHT|DIFF|ROUGH_COND (config 3a), without a medium: every microfacet distribution, and GGX alone (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_ROUGH_COND(PT_INSTANTIATE_VARIANT) }
