// pt_kernel_aov.hip -- the guide kernels of pt_render_aov (first-hit albedo, normal, depth, coverage): pt_aov_first.h around the device
// functions of pt_trace.h (node4_step, ray_inv, leaf_test, closest_hit, gen_camera_ray, the record and texture fetches), and none of the
// render or probe kernels.  Moeller-Trumbore; the watertight instances are pt_kernel_aov_wt.hip.
#include "pt_aov_first.h"
