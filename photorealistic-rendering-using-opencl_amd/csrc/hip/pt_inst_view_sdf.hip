// pt_inst_view_sdf.hip -- render_kernel for the debug views of H_SDF scenes, medium off / on (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_VIEW_SDF(PT_INSTANTIATE_VARIANT) }
