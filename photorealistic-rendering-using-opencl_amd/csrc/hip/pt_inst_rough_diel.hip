// pt_inst_rough_diel.hip -- render_kernel for the material set LIGHT|DIFF|DIEL|ROUGH_DIEL (config 3b), without a medium: every microfacet distribution, and GGX alone (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_ROUGH_DIEL(PT_INSTANTIATE_VARIANT) }
