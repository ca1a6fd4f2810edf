// pt_inst_light_diff.hip -- render_kernel for the material set LIGHT|DIFF (configs 2, 4, 5: Lambert + light), medium off / on (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_LIGHT_DIFF(PT_INSTANTIATE_VARIANT) }
