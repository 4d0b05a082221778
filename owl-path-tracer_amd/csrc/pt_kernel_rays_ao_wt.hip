// pt_kernel_rays_ao_wt.hip -- the watertight instances of the fused ambient-occlusion kernel (pt_trace_ao under option "watertight" = 1):
// pt_ao.h with PT_WATERTIGHT = 1.
#define PT_WATERTIGHT 1
#include "pt_ao.h"
