// pt_inst_view.hip -- render_kernel for the debug views VIEW_NORMAL / VIEW_BVH_HIT, medium off / on (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_VIEW(PT_INSTANTIATE_VARIANT) }
