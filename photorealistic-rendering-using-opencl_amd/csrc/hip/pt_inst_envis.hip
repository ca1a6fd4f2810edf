// pt_inst_envis.hip -- render_kernel for environment-map importance sampling (prt_config::env_importance_sampling), surfaces only (rows: pt_variant.h)
#include "pt_render.h"
namespace prt { PT_VARIANTS_ENVIS(PT_INSTANTIATE_VARIANT) }
