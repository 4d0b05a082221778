// pt_kernel_rays_wt.hip -- the watertight instances of the ray kernels (pt_trace_closest / pt_trace_occluded under option "watertight" = 1):
// pt_rays_kernels.h with PT_WATERTIGHT = 1 (leaf_test is then the watertight test of pt_trace.h).
#define PT_WATERTIGHT 1
#include "pt_rays_kernels.h"
