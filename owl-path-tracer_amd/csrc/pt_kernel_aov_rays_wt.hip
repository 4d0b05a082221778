// pt_kernel_aov_rays_wt.hip -- the watertight ray-image instances of the follow kernels (pt_render_aov_rays under option "watertight" = 1):
// pt_aov_follow.h with PT_RAYGEN = 1 and PT_WATERTIGHT = 1 (pt_aov_rays_wt_kernel behind pt_launch_aov_rays_wt / pt_aov_rays_geometry_wt).
#define PT_RAYGEN 1
#define PT_WATERTIGHT 1
#include "pt_aov_follow.h"
