// pt_inst_generic.hip -- render_kernel for any other ACTIVE_MATS (the materials dispatched at run time), medium off / on (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_GENERIC(PT_INSTANTIATE_VARIANT) }
