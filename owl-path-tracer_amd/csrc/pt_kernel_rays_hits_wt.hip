// pt_kernel_rays_hits_wt.hip -- the watertight instances of the first-K-hits kernel (pt_trace_hits under option "watertight" = 1):
// pt_hits.h with PT_WATERTIGHT = 1.
#define PT_WATERTIGHT 1
#include "pt_hits.h"
