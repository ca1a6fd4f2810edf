// pt_inst_pick.hip -- render_kernel for PICK_RANDOM_LIGHT (prt_config::pick_random_light), medium off / on (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_PICK(PT_INSTANTIATE_VARIANT) }
