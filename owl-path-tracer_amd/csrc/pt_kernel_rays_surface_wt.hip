// pt_kernel_rays_surface_wt.hip -- the watertight surface instances of the ray kernels (pt_trace_surface under option "watertight" = 1):
// pt_rays_kernels.h with PT_RAYS_SURFACE = 1 and PT_WATERTIGHT = 1.
#define PT_RAYS_SURFACE 1
#define PT_WATERTIGHT 1
#include "pt_rays_kernels.h"
