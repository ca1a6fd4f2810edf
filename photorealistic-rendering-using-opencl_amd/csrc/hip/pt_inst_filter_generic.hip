// pt_inst_filter_generic.hip -- render_kernel for the run-time dispatch under a pixel filter, medium off / on (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_FILTER_GENERIC(PT_INSTANTIATE_VARIANT) }
