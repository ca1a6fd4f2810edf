// pt_inst_sdf.hip -- render_kernel for H_SDF scenes (the run-time dispatch with the raymarcher), medium off / on (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_SDF(PT_INSTANTIATE_VARIANT) }
