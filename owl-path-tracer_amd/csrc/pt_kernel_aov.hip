// pt_kernel_aov.hip -- the guide kernels of pt_render_aov (first-hit albedo, normal, depth, coverage): pt_kernel.hip with PT_AOV = 1,
// i.e. its device functions (node4_step, and through pt_trace.h ray_inv, leaf_test, closest_hit, gen_camera_ray, the record and texture
// fetches) around pt_aov_kernel and its launcher, and none of the render or probe kernels.  Moeller-Trumbore; the watertight instances
// are pt_kernel_aov_wt.hip.
#define PT_AOV 1
#include "pt_kernel.hip"
