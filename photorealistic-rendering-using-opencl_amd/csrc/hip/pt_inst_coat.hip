// pt_inst_coat.hip -- render_kernel for the material set LIGHT|DIFF|COAT (scenes/cornell.json as shipped (config 1)), without a medium: every microfacet distribution, and Beckmann alone (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_COAT(PT_INSTANTIATE_VARIANT) }
