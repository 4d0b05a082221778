// pt_kernel_aov_rays.hip -- the ray-image instances of the follow kernels (pt_render_aov_rays): pt_aov_follow.h with PT_RAYGEN = 1, as
// pt_kernel_rayimage.hip is pt_kernel.hip with it - every sample starts on the pixel's ray record of the caller's table (gen_ray_from,
// pt_trace.h; the table travels in P.batch_cams) instead of a camera's ray, and everything behind that ray is the follow kernel's.
// pt_aov_rays_kernel behind pt_launch_aov_rays / pt_aov_rays_geometry; quad walk only.  Moeller-Trumbore; the watertight instances are
// pt_kernel_aov_rays_wt.hip.  A translation unit of its own, so that `make asm-aov-follow` goes on listing its five kernels.
#define PT_RAYGEN 1
#include "pt_aov_follow.h"
